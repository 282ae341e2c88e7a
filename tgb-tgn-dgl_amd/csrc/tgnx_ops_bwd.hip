// Backward (and the two remaining forward) per-operator entry points: what makes the operators of tgnx_ops.hip
// trainable from torch (tgnx/ops.py autograd functions, tgnx/nn.py modules).  The fused train steps do not call
// these.  Every contraction runs on tgnx_gemm_f32; the kernels here are the elementwise and reduction parts.
//
//   tgnx_col_sum                 bias gradients (column sums in a fixed order)
//   tgnx_memory_cell_bwd         GRUCell / RNNCell backward          modules/memory_module.py:70-78
//   tgnx_link_predictor_bwd      LinkPredictor / EdgePredictor       modules/decoder.py:12-27, model_utils.py:165-195
//   tgnx_time_encode (+ _bwd)    TimeEncoder cos(w t + b)            [ext] torch_geometric TimeEncoder
//   tgnx_time_embedding (+ _bwd) TimeEmbedding x (1 + w rel_t + b)   modules/emb_module.py:32-52
//   tgnx_msg_agg_last_bwd / tgnx_msg_agg_mean_bwd                    modules/msg_agg.py:15-26
//
// Determinism: no float atomics.  Column reductions run in a fixed order that depends on the shape alone (below);
// the per-destination sums walk their rows in increasing order; the only atomics are integer counts.
#include <math.h>

#include <algorithm>

#include "tgnx_common.h"
#include "tgnx_math.h"

using namespace tgnx;

namespace {

constexpr int OPS_BLOCK = 256;
constexpr int WAVES = OPS_BLOCK / WAVE;

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------ column reductions
// out[c] = Σ_m f(m, c) for up to two outputs at once.  The rows are cut into chunks of CS_ROWS; a workgroup owns
// (chunk, 64-column strip): lane = column (a wave reads 256 contiguous bytes of a row), wave w walks rows
// w, w + 4, ... of the chunk sequentially, the four waves' partials are added in wave order through LDS.  One
// chunk writes `out` directly; more chunks write partials [chunk][N] that col_finish adds in chunk order.  The
// order is a function of (M, N) only.
constexpr int CS_ROWS = 256;
constexpr int64_t CS_MAX_N = int64_t(65535) * WAVE;  // strips ride gridDim.y

int64_t cs_chunks(int64_t M) { return std::max<int64_t>(ceil_div(M, CS_ROWS), 1); }
// bytes of partials for `nout` outputs (none with a single chunk; never 0 so that a workspace pointer exists)
size_t cs_bytes(int64_t M, int64_t N, int nout) {
  const int64_t nc = cs_chunks(M);
  if (nc <= 1 || N <= 0) return 256;
  return nout * align256((size_t)nc * N * 4);
}

template <class F>
__global__ void __launch_bounds__(OPS_BLOCK) col_reduce(int64_t M, int64_t N, F f, float* p0, float* p1) {
  __shared__ float sa[WAVES][WAVE], sb[WAVES][WAVE];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t chunk = blockIdx.x, c = blockIdx.y * (int64_t)WAVE + lane;
  const int64_t r0 = chunk * CS_ROWS, r1 = min(M, r0 + CS_ROWS);
  float a = 0.f, b = 0.f;
  if (c < N)
    for (int64_t m = r0 + w; m < r1; m += WAVES) {
      float va = 0.f, vb = 0.f;
      f(m, c, va, vb);
      a += va;
      b += vb;
    }
  sa[w][lane] = a;
  sb[w][lane] = b;
  __syncthreads();
  if (w == 0 && c < N) {
    a = sa[0][lane];
    b = sb[0][lane];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) {
      a += sa[k][lane];
      b += sb[k][lane];
    }
    if (p0) p0[chunk * N + c] = a;
    if (p1) p1[chunk * N + c] = b;
  }
}

__global__ void __launch_bounds__(OPS_BLOCK) col_finish(int64_t nc, int64_t N, const float* p0, const float* p1,
                                                        float* o0, float* o1) {
  const int64_t c = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (c >= N) return;
  if (o0) {
    float s = 0.f;
    for (int64_t k = 0; k < nc; ++k) s += p0[k * N + c];
    o0[c] = s;
  }
  if (o1) {
    float s = 0.f;
    for (int64_t k = 0; k < nc; ++k) s += p1[k * N + c];
    o1[c] = s;
  }
}

// o0 / o1 (either may be NULL) = the column sums of f's two values; ws: cs_bytes(M, N, 2) bytes
template <class F>
int col_reduce_launch(int64_t M, int64_t N, F f, float* o0, float* o1, void* ws, hipStream_t s) {
  if (N == 0 || (!o0 && !o1)) return TGNX_OK;
  if (M == 0) {
    if (o0) TGNX_HIP_CHECK(hipMemsetAsync(o0, 0, N * 4, s));
    if (o1) TGNX_HIP_CHECK(hipMemsetAsync(o1, 0, N * 4, s));
    return TGNX_OK;
  }
  const int64_t nc = cs_chunks(M);
  const dim3 grid((unsigned)nc, (unsigned)ceil_div(N, WAVE));
  if (nc == 1) {
    hipLaunchKernelGGL(col_reduce<F>, grid, dim3(OPS_BLOCK), 0, s, M, N, f, o0, o1);
    TGNX_LAUNCH_CHECK("col_reduce");
    return TGNX_OK;
  }
  float* p0 = reinterpret_cast<float*>(ws);
  float* p1 = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + align256((size_t)nc * N * 4));
  hipLaunchKernelGGL(col_reduce<F>, grid, dim3(OPS_BLOCK), 0, s, M, N, f, o0 ? p0 : nullptr, o1 ? p1 : nullptr);
  TGNX_LAUNCH_CHECK("col_reduce");
  hipLaunchKernelGGL(col_finish, dim3((unsigned)ceil_div(N, OPS_BLOCK)), dim3(OPS_BLOCK), 0, s, nc, N,
                     (const float*)p0, (const float*)p1, o0, o1);
  TGNX_LAUNCH_CHECK("col_finish");
  return TGNX_OK;
}

struct SumF {  // plain column sum of x [M, N] (row stride ldx)
  const float* x;
  int64_t ldx;
  __device__ void operator()(int64_t m, int64_t c, float& a, float&) const { a = x[m * ldx + c]; }
};

// ------------------------------------------------------------------ memory cell backward
// gi / gh hold the recomputed pre-activations on entry and dgi / dgh on return (in place: element (m, d) of each
// gate chunk is read and written by the one thread that owns (m, d)).  GRU, torch's r, z, n chunks:
//   dn = dh'(1 − z), dz = dh'(h − n), dh = dh' z, dn_pre = dn (1 − n²), dr_pre = dn_pre gh_n r (1 − r),
//   dz_pre = dz z (1 − z); dgi = [dr_pre, dz_pre, dn_pre], dgh = [dr_pre, dz_pre, dn_pre r].
// RNN (tanh): dgi = dgh = dh'(1 − h'²), written to gi only; no direct dh term.
__global__ void __launch_bounds__(OPS_BLOCK) cell_gates_bwd(int cell, int64_t M, int64_t D, const float* dh_out,
                                                            const float* h, float* gi, float* gh, float* dh) {
  const int64_t x = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (x >= M * D) return;
  const float g = dh_out[x];
  if (cell == 1) {
    const float hn = tanhf(gi[x] + gh[x]);
    gi[x] = g * (1.f - hn * hn);
    return;
  }
  const int64_t m = x / D, d = x % D;
  float* a = gi + m * 3 * D;
  float* b = gh + m * 3 * D;
  const float ghn = b[2 * D + d];
  const float r = sigm(a[d] + b[d]);
  const float z = sigm(a[D + d] + b[D + d]);
  const float n = tanhf(a[2 * D + d] + r * ghn);
  const float dn_pre = g * (1.f - z) * (1.f - n * n);
  const float dr_pre = dn_pre * ghn * (r * (1.f - r));
  const float dz_pre = g * (h[x] - n) * (z * (1.f - z));
  a[d] = dr_pre;
  a[D + d] = dz_pre;
  a[2 * D + d] = dn_pre;
  b[d] = dr_pre;
  b[D + d] = dz_pre;
  b[2 * D + d] = dn_pre * r;
  if (dh) dh[x] = g * z;
}

size_t cell_bwd_gemm_bytes(int64_t M, int64_t d_in, int64_t D) {
  const int64_t G = 3 * D;
  size_t g = std::max(tgnx_gemm_f32_ws_bytes(M, G, d_in), tgnx_gemm_f32_ws_bytes(M, G, D));
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(M, d_in, G), tgnx_gemm_f32_ws_bytes(M, D, G)));
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(G, d_in, M), tgnx_gemm_f32_ws_bytes(G, D, M)));
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(M, D, d_in), tgnx_gemm_f32_ws_bytes(M, D, D)));
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(M, d_in, D), tgnx_gemm_f32_ws_bytes(D, d_in, M)));
  return std::max(g, tgnx_gemm_f32_ws_bytes(D, D, M));
}

// ------------------------------------------------------------------ link predictor backward
// A wave per output row i: the recomputed out_i gives g_i = dout_i (· σ(1 − σ) with the sigmoid), stored for the
// w_out / b_out sums, and da[i, c] = g_i w_out[c] [hs[i mod n_src, c] + hd[i, c] > 0].
__global__ void __launch_bounds__(OPS_BLOCK) pred_rows_bwd(int64_t n_src, int64_t M, int64_t D, const float* dout,
                                                           const float* hs, const float* hd, const float* w_out,
                                                           const float* b_out, int sigmoid, float* g, float* da) {
  const int64_t i = blockIdx.x * (int64_t)WAVES + (threadIdx.x >> 6);
  if (i >= M) return;
  const int lane = threadIdx.x & 63;
  const float* a = hs + (i % n_src) * D;
  const float* b = hd + i * D;
  float gi = dout[i];
  if (sigmoid) {
    float s = 0.f;
    for (int64_t c = lane; c < D; c += WAVE) s += w_out[c] * fmaxf(a[c] + b[c], 0.f);
    const float y = sigm(wave_sum(s) + b_out[0]);
    gi *= y * (1.f - y);
  }
  if (lane == 0) g[i] = gi;
  for (int64_t c = lane; c < D; c += WAVE) da[i * D + c] = (a[c] + b[c] > 0.f) ? gi * w_out[c] : 0.f;
}

// dhs[j] = Σ_{i ≡ j (mod n_src)} da[i], in increasing i (the `tile` pairing's transpose)
__global__ void __launch_bounds__(OPS_BLOCK) pred_tile_sum(int64_t n_src, int64_t M, int64_t D, const float* da,
                                                           float* dhs) {
  const int64_t x = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (x >= n_src * D) return;
  const int64_t j = x / D, c = x % D;
  float s = 0.f;
  for (int64_t i = j; i < M; i += n_src) s += da[i * D + c];
  dhs[x] = s;
}

struct PredWoutF {  // dw_out[c] = Σ_i g_i relu(hs[i mod n_src, c] + hd[i, c])
  const float *g, *hs, *hd;
  int64_t n_src, D;
  __device__ void operator()(int64_t m, int64_t c, float& a, float&) const {
    a = g[m] * fmaxf(hs[(m % n_src) * D + c] + hd[m * D + c], 0.f);
  }
};

size_t pred_bwd_gemm_bytes(int64_t n_src, int64_t M, int64_t d_in, int64_t D) {
  size_t g = std::max(tgnx_gemm_f32_ws_bytes(n_src, D, d_in), tgnx_gemm_f32_ws_bytes(M, D, d_in));
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(n_src, d_in, D), tgnx_gemm_f32_ws_bytes(M, d_in, D)));
  return std::max(g, std::max(tgnx_gemm_f32_ws_bytes(D, d_in, n_src), tgnx_gemm_f32_ws_bytes(D, d_in, M)));
}

// ------------------------------------------------------------------ time encoder / time embedding
__global__ void __launch_bounds__(OPS_BLOCK) time_encode_k(int64_t n, int64_t D, const float* t, const float* w,
                                                           const float* b, float* out) {
  const int64_t x = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (x >= n * D) return;
  const int64_t c = x % D;
  out[x] = te_cos(fmaf(w[c], t[x / D], b[c]));
}

struct TimeEncBwdF {  // dw[c] = Σ_n −sin(·) t[n] dout[n, c];  db[c] = Σ_n −sin(·) dout[n, c]
  const float *t, *w, *b, *dout;
  int64_t D;
  __device__ void operator()(int64_t m, int64_t c, float& a, float& bb) const {
    float sn, cs;
    const float tm = t[m];
    te_sincos(fmaf(w[c], tm, b[c]), sn, cs);
    bb = -sn * dout[m * D + c];
    a = bb * tm;
  }
};

// out = x (1 + (w rel_t + b)); with dout: dx = dout (1 + (w rel_t + b))
__global__ void __launch_bounds__(OPS_BLOCK) time_embedding_k(int64_t n, int64_t D, const float* x,
                                                              const float* rel_t, const float* w, const float* b,
                                                              float* out) {
  const int64_t i = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (i >= n * D) return;
  const int64_t c = i % D;
  out[i] = x[i] * (1.f + (w[c] * rel_t[i / D] + b[c]));
}

struct TimeEmbBwdF {  // dw[c] = Σ_n dout x rel_t;  db[c] = Σ_n dout x
  const float *x, *rel_t, *dout;
  int64_t D;
  __device__ void operator()(int64_t m, int64_t c, float& a, float& bb) const {
    bb = dout[m * D + c] * x[m * D + c];
    a = bb * rel_t[m];
  }
};

// ------------------------------------------------------------------ message aggregation backward
// last: a wave per output row copies dout[r] to dmsg[argmax[r]] (distinct rows have distinct argmax; dmsg zeroed)
__global__ void __launch_bounds__(OPS_BLOCK) agg_last_bwd(const float* dout, const int64_t* argmax,
                                                          int64_t dim_size, int64_t dim, int64_t n_msg,
                                                          float* dmsg) {
  const int64_t r = blockIdx.x * (int64_t)WAVES + (threadIdx.x >> 6);
  if (r >= dim_size) return;
  const int64_t a = argmax[r];
  if (a < 0 || a >= n_msg) return;
  const int lane = threadIdx.x & 63;
  for (int64_t c = lane; c < dim; c += WAVE) dmsg[a * dim + c] = dout[r * dim + c];
}

// mean: integer histogram of the index, then dmsg[p] = dout[index[p]] / count
__global__ void __launch_bounds__(OPS_BLOCK) agg_count(const int64_t* index, int64_t n, int64_t dim_size, int* cnt,
                                                       int64_t* n_invalid) {
  const int64_t p = blockIdx.x * (int64_t)OPS_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t k = index[p];
  if (k >= 0 && k < dim_size) atomicAdd(cnt + k, 1);
  else if (n_invalid) atomicAdd(reinterpret_cast<unsigned long long*>(n_invalid), 1ull);
}

__global__ void __launch_bounds__(OPS_BLOCK) agg_mean_bwd(const float* dout, const int64_t* index, const int* cnt,
                                                          int64_t n, int64_t dim, int64_t dim_size, float* dmsg) {
  const int64_t p = blockIdx.x * (int64_t)WAVES + (threadIdx.x >> 6);
  if (p >= n) return;
  const int lane = threadIdx.x & 63;
  const int64_t k = index[p];
  const bool ok = k >= 0 && k < dim_size;
  const float c = ok ? (float)cnt[k] : 1.f;
  for (int64_t x = lane; x < dim; x += WAVE) dmsg[p * dim + x] = ok ? __fdiv_rn(dout[k * dim + x], c) : 0.f;
}

}  // namespace

extern "C" {

size_t tgnx_col_sum_ws_bytes(int64_t M, int64_t N) {
  if (M < 0 || N < 0) return 0;
  return cs_bytes(M, N, 1);
}

int tgnx_col_sum(int64_t M, int64_t N, const float* x, int64_t ldx, float* out, void* ws, size_t ws_bytes,
                 void* stream) {
  TGNX_CHECK_ARG(M >= 0 && N >= 0 && M < (int64_t(1) << 38) && N <= CS_MAX_N && ldx >= N,
                 "tgnx_col_sum: bad sizes (ldx >= N)");
  if (N == 0) return TGNX_OK;
  TGNX_CHECK_ARG(out && ws && (M == 0 || x), "tgnx_col_sum: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_col_sum_ws_bytes(M, N), "tgnx_col_sum: workspace too small");
  return col_reduce_launch(M, N, SumF{x, ldx}, out, nullptr, ws, as_stream(stream));
}

size_t tgnx_memory_cell_bwd_ws_bytes(int64_t M, int64_t d_in, int64_t D) {
  if (M <= 0 || d_in <= 0 || D <= 0) return 256;
  return 2 * align256(M * 3 * D * 4) + align256(cell_bwd_gemm_bytes(M, d_in, D)) + cs_bytes(M, 3 * D, 1);
}

int tgnx_memory_cell_bwd(int32_t cell, int64_t M, int64_t d_in, int64_t D, const float* dh_out, const float* x,
                         const float* h, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                         float* dx, float* dh, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* ws,
                         size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(cell == 0 || cell == 1, "tgnx_memory_cell_bwd: cell must be 0 (GRUCell) or 1 (RNNCell, tanh)");
  TGNX_CHECK_ARG(M >= 0 && d_in > 0 && D > 0 && M < (1 << 30) && d_in < (1 << 30) && D < (1 << 28),
                 "tgnx_memory_cell_bwd: bad sizes");
  const int64_t G = (cell == 0 ? 3 : 1) * D;
  hipStream_t s = as_stream(stream);
  if (M == 0) {  // no rows: the parameter gradients are zero
    if (dw_ih) TGNX_HIP_CHECK(hipMemsetAsync(dw_ih, 0, G * d_in * 4, s));
    if (dw_hh) TGNX_HIP_CHECK(hipMemsetAsync(dw_hh, 0, G * D * 4, s));
    if (db_ih) TGNX_HIP_CHECK(hipMemsetAsync(db_ih, 0, G * 4, s));
    if (db_hh) TGNX_HIP_CHECK(hipMemsetAsync(db_hh, 0, G * 4, s));
    return TGNX_OK;
  }
  TGNX_CHECK_ARG(dh_out && x && h && w_ih && w_hh && ws, "tgnx_memory_cell_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_memory_cell_bwd_ws_bytes(M, d_in, D), "tgnx_memory_cell_bwd: workspace too small");
  char* p = reinterpret_cast<char*>(ws);
  const size_t gate_bytes = align256(M * 3 * D * 4), gemm_bytes = align256(cell_bwd_gemm_bytes(M, d_in, D));
  float* gi = reinterpret_cast<float*>(p);
  float* gh = reinterpret_cast<float*>(p + gate_bytes);
  void* gws = p + 2 * gate_bytes;
  void* cws = p + 2 * gate_bytes + gemm_bytes;
  int rc = tgnx_gemm_f32(M, G, d_in, x, d_in, 0, w_ih, d_in, 1, gi, G, b_ih, 0, gws, gemm_bytes, stream);
  if (rc != TGNX_OK) return rc;
  rc = tgnx_gemm_f32(M, G, D, h, D, 0, w_hh, D, 1, gh, G, b_hh, 0, gws, gemm_bytes, stream);
  if (rc != TGNX_OK) return rc;
  hipLaunchKernelGGL(cell_gates_bwd, dim3((unsigned)ceil_div(M * D, OPS_BLOCK)), dim3(OPS_BLOCK), 0, s, (int)cell, M,
                     D, dh_out, h, gi, gh, dh);
  TGNX_LAUNCH_CHECK("cell_gates_bwd");
  const float* dgi = gi;
  const float* dgh = cell == 0 ? gh : gi;
  if (dx) {  // dx = dgi W_ih
    rc = tgnx_gemm_f32(M, d_in, G, dgi, G, 0, w_ih, d_in, 0, dx, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dh) {  // dh (+)= dgh W_hh: on top of the GRU's direct term dh' z
    rc = tgnx_gemm_f32(M, D, G, dgh, G, 0, w_hh, D, 0, dh, D, nullptr, cell == 0 ? 1 : 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dw_ih) {  // dW_ih = dgi^T x
    rc = tgnx_gemm_f32(G, d_in, M, dgi, G, 1, x, d_in, 0, dw_ih, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dw_hh) {  // dW_hh = dgh^T h
    rc = tgnx_gemm_f32(G, D, M, dgh, G, 1, h, D, 0, dw_hh, D, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  rc = col_reduce_launch(M, G, SumF{dgi, G}, db_ih, nullptr, cws, s);
  if (rc != TGNX_OK) return rc;
  return col_reduce_launch(M, G, SumF{dgh, G}, db_hh, nullptr, cws, s);
}

size_t tgnx_link_predictor_bwd_ws_bytes(int64_t n_src, int64_t M, int64_t d_in, int64_t D) {
  if (n_src <= 0 || M <= 0 || d_in <= 0 || D <= 0) return 256;
  return 2 * align256(n_src * D * 4) + 2 * align256(M * D * 4) + align256(M * 4) +
         align256(pred_bwd_gemm_bytes(n_src, M, d_in, D)) + cs_bytes(std::max(M, n_src), D, 1);
}

int tgnx_link_predictor_bwd(int64_t n_src, int64_t M, int64_t d_in, int64_t D, const float* dout, const float* z_src,
                            const float* z_dst, const float* w_src, const float* b_src, const float* w_dst,
                            const float* b_dst, const float* w_out, const float* b_out, int32_t sigmoid,
                            float* dz_src, float* dz_dst, float* dw_src, float* db_src, float* dw_dst, float* db_dst,
                            float* dw_out, float* db_out, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(n_src >= 0 && M >= 0 && d_in > 0 && D > 0 && n_src < (1 << 30) && M < (1 << 30) &&
                     d_in < (1 << 30) && D < (1 << 30),
                 "tgnx_link_predictor_bwd: bad sizes");
  TGNX_CHECK_ARG(M == 0 || n_src > 0, "tgnx_link_predictor_bwd: rows to predict but no source rows");
  hipStream_t s = as_stream(stream);
  if (M == 0) {  // nothing predicted: every gradient is zero
    if (dz_src && n_src) TGNX_HIP_CHECK(hipMemsetAsync(dz_src, 0, n_src * d_in * 4, s));
    if (dw_src) TGNX_HIP_CHECK(hipMemsetAsync(dw_src, 0, D * d_in * 4, s));
    if (dw_dst) TGNX_HIP_CHECK(hipMemsetAsync(dw_dst, 0, D * d_in * 4, s));
    if (db_src) TGNX_HIP_CHECK(hipMemsetAsync(db_src, 0, D * 4, s));
    if (db_dst) TGNX_HIP_CHECK(hipMemsetAsync(db_dst, 0, D * 4, s));
    if (dw_out) TGNX_HIP_CHECK(hipMemsetAsync(dw_out, 0, D * 4, s));
    if (db_out) TGNX_HIP_CHECK(hipMemsetAsync(db_out, 0, 4, s));
    return TGNX_OK;
  }
  TGNX_CHECK_ARG(dout && z_src && z_dst && w_src && w_dst && w_out && b_out && ws,
                 "tgnx_link_predictor_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_link_predictor_bwd_ws_bytes(n_src, M, d_in, D),
                 "tgnx_link_predictor_bwd: workspace too small");
  char* p = reinterpret_cast<char*>(ws);
  const size_t sb = align256(n_src * D * 4), mb = align256(M * D * 4);
  const size_t gemm_bytes = align256(pred_bwd_gemm_bytes(n_src, M, d_in, D));
  float* hs = reinterpret_cast<float*>(p);
  float* dhs = reinterpret_cast<float*>(p + sb);
  float* hd = reinterpret_cast<float*>(p + 2 * sb);
  float* da = reinterpret_cast<float*>(p + 2 * sb + mb);
  float* g = reinterpret_cast<float*>(p + 2 * sb + 2 * mb);
  void* gws = p + 2 * sb + 2 * mb + align256(M * 4);
  void* cws = p + 2 * sb + 2 * mb + align256(M * 4) + gemm_bytes;
  int rc = tgnx_gemm_f32(n_src, D, d_in, z_src, d_in, 0, w_src, d_in, 1, hs, D, b_src, 0, gws, gemm_bytes, stream);
  if (rc != TGNX_OK) return rc;
  rc = tgnx_gemm_f32(M, D, d_in, z_dst, d_in, 0, w_dst, d_in, 1, hd, D, b_dst, 0, gws, gemm_bytes, stream);
  if (rc != TGNX_OK) return rc;
  hipLaunchKernelGGL(pred_rows_bwd, dim3((unsigned)ceil_div(M, WAVES)), dim3(OPS_BLOCK), 0, s, n_src, M, D, dout,
                     (const float*)hs, (const float*)hd, w_out, b_out, (int)sigmoid, g, da);
  TGNX_LAUNCH_CHECK("pred_rows_bwd");
  if (dz_src || dw_src || db_src) {
    hipLaunchKernelGGL(pred_tile_sum, dim3((unsigned)ceil_div(n_src * D, OPS_BLOCK)), dim3(OPS_BLOCK), 0, s, n_src, M,
                       D, (const float*)da, dhs);
    TGNX_LAUNCH_CHECK("pred_tile_sum");
  }
  rc = col_reduce_launch(M, D, PredWoutF{g, hs, hd, n_src, D}, dw_out, nullptr, cws, s);
  if (rc != TGNX_OK) return rc;
  rc = col_reduce_launch(M, 1, SumF{g, 1}, db_out, nullptr, cws, s);
  if (rc != TGNX_OK) return rc;
  if (dz_src) {  // dz_src = dhs W_src
    rc = tgnx_gemm_f32(n_src, d_in, D, dhs, D, 0, w_src, d_in, 0, dz_src, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dz_dst) {  // dz_dst = da W_dst
    rc = tgnx_gemm_f32(M, d_in, D, da, D, 0, w_dst, d_in, 0, dz_dst, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dw_src) {  // dW_src = dhs^T z_src
    rc = tgnx_gemm_f32(D, d_in, n_src, dhs, D, 1, z_src, d_in, 0, dw_src, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dw_dst) {  // dW_dst = da^T z_dst
    rc = tgnx_gemm_f32(D, d_in, M, da, D, 1, z_dst, d_in, 0, dw_dst, d_in, nullptr, 0, gws, gemm_bytes, stream);
    if (rc != TGNX_OK) return rc;
  }
  rc = col_reduce_launch(n_src, D, SumF{dhs, D}, db_src, nullptr, cws, s);
  if (rc != TGNX_OK) return rc;
  return col_reduce_launch(M, D, SumF{da, D}, db_dst, nullptr, cws, s);
}

int tgnx_time_encode(int64_t n, int64_t D, const float* t, const float* w, const float* b, float* out, void* stream) {
  TGNX_CHECK_ARG(n >= 0 && D >= 0 && n < (int64_t(1) << 40) && D < (1 << 30) && n * D < (int64_t(1) << 40),
                 "tgnx_time_encode: bad sizes");
  if (n == 0 || D == 0) return TGNX_OK;
  TGNX_CHECK_ARG(t && w && b && out, "tgnx_time_encode: null pointer");
  hipLaunchKernelGGL(time_encode_k, dim3((unsigned)ceil_div(n * D, OPS_BLOCK)), dim3(OPS_BLOCK), 0, as_stream(stream),
                     n, D, t, w, b, out);
  TGNX_LAUNCH_CHECK("time_encode");
  return TGNX_OK;
}

size_t tgnx_time_encode_bwd_ws_bytes(int64_t n, int64_t D) {
  if (n < 0 || D < 0) return 0;
  return cs_bytes(n, D, 2);
}

int tgnx_time_encode_bwd(int64_t n, int64_t D, const float* t, const float* w, const float* b, const float* dout,
                         float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(n >= 0 && D >= 0 && n < (int64_t(1) << 38) && D <= CS_MAX_N, "tgnx_time_encode_bwd: bad sizes");
  if (D == 0) return TGNX_OK;
  TGNX_CHECK_ARG(ws && (n == 0 || (t && w && b && dout)), "tgnx_time_encode_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_time_encode_bwd_ws_bytes(n, D), "tgnx_time_encode_bwd: workspace too small");
  return col_reduce_launch(n, D, TimeEncBwdF{t, w, b, dout, D}, dw, db, ws, as_stream(stream));
}

int tgnx_time_embedding(int64_t n, int64_t D, const float* x, const float* rel_t, const float* w, const float* b,
                        float* out, void* stream) {
  TGNX_CHECK_ARG(n >= 0 && D >= 0 && n < (int64_t(1) << 40) && D < (1 << 30) && n * D < (int64_t(1) << 40),
                 "tgnx_time_embedding: bad sizes");
  if (n == 0 || D == 0) return TGNX_OK;
  TGNX_CHECK_ARG(x && rel_t && w && b && out, "tgnx_time_embedding: null pointer");
  hipLaunchKernelGGL(time_embedding_k, dim3((unsigned)ceil_div(n * D, OPS_BLOCK)), dim3(OPS_BLOCK), 0,
                     as_stream(stream), n, D, x, rel_t, w, b, out);
  TGNX_LAUNCH_CHECK("time_embedding");
  return TGNX_OK;
}

size_t tgnx_time_embedding_bwd_ws_bytes(int64_t n, int64_t D) {
  if (n < 0 || D < 0) return 0;
  return cs_bytes(n, D, 2);
}

int tgnx_time_embedding_bwd(int64_t n, int64_t D, const float* x, const float* rel_t, const float* w, const float* b,
                            const float* dout, float* dx, float* dw, float* db, void* ws, size_t ws_bytes,
                            void* stream) {
  TGNX_CHECK_ARG(n >= 0 && D >= 0 && n < (int64_t(1) << 38) && D <= CS_MAX_N && n * D < (int64_t(1) << 40),
                 "tgnx_time_embedding_bwd: bad sizes");
  if (D == 0) return TGNX_OK;
  TGNX_CHECK_ARG(ws && (n == 0 || (x && rel_t && w && b && dout)), "tgnx_time_embedding_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_time_embedding_bwd_ws_bytes(n, D), "tgnx_time_embedding_bwd: workspace too small");
  hipStream_t s = as_stream(stream);
  if (dx && n > 0) {  // dx = dout (1 + w rel_t + b): the forward's kernel on dout
    hipLaunchKernelGGL(time_embedding_k, dim3((unsigned)ceil_div(n * D, OPS_BLOCK)), dim3(OPS_BLOCK), 0, s, n, D, dout,
                       rel_t, w, b, dx);
    TGNX_LAUNCH_CHECK("time_embedding_bwd");
  }
  return col_reduce_launch(n, D, TimeEmbBwdF{x, rel_t, dout, D}, dw, db, ws, s);
}

int tgnx_msg_agg_last_bwd(const float* dout, const int64_t* argmax, int64_t dim_size, int64_t dim, int64_t n_msg,
                          float* dmsg, void* stream) {
  TGNX_CHECK_ARG(n_msg >= 0 && dim >= 0 && dim_size >= 0 && n_msg < (int64_t(1) << 40) &&
                     dim_size < (int64_t(1) << 32) && dim < (1 << 30) && n_msg * dim < (int64_t(1) << 40),
                 "tgnx_msg_agg_last_bwd: bad sizes");
  if (n_msg == 0 || dim == 0) return TGNX_OK;
  TGNX_CHECK_ARG(dmsg && (dim_size == 0 || (dout && argmax)), "tgnx_msg_agg_last_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(dmsg, 0, n_msg * dim * 4, s));
  if (dim_size == 0) return TGNX_OK;
  hipLaunchKernelGGL(agg_last_bwd, dim3((unsigned)ceil_div(dim_size, WAVES)), dim3(OPS_BLOCK), 0, s, dout, argmax,
                     dim_size, dim, n_msg, dmsg);
  TGNX_LAUNCH_CHECK("agg_last_bwd");
  return TGNX_OK;
}

size_t tgnx_msg_agg_mean_bwd_ws_bytes(int64_t dim_size) {
  if (dim_size < 0) return 0;
  return std::max<size_t>(align256((size_t)dim_size * 4), 256);
}

int tgnx_msg_agg_mean_bwd(const float* dout, const int64_t* index, int64_t n_msg, int64_t dim, int64_t dim_size,
                          float* dmsg, int64_t* n_invalid, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(n_msg >= 0 && dim >= 0 && dim_size >= 0 && n_msg < (int64_t(1) << 32) &&
                     dim_size < (int64_t(1) << 40) && dim < (1 << 30) && n_msg * dim < (int64_t(1) << 40),
                 "tgnx_msg_agg_mean_bwd: bad sizes");
  if (n_msg == 0) return TGNX_OK;
  TGNX_CHECK_ARG(index && ws && (dim == 0 || dmsg) && (dim_size == 0 || dim == 0 || dout),
                 "tgnx_msg_agg_mean_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_msg_agg_mean_bwd_ws_bytes(dim_size), "tgnx_msg_agg_mean_bwd: workspace too small");
  hipStream_t s = as_stream(stream);
  int* cnt = reinterpret_cast<int*>(ws);
  if (dim_size > 0) TGNX_HIP_CHECK(hipMemsetAsync(cnt, 0, dim_size * 4, s));
  hipLaunchKernelGGL(agg_count, dim3((unsigned)ceil_div(n_msg, OPS_BLOCK)), dim3(OPS_BLOCK), 0, s, index, n_msg,
                     dim_size, cnt, n_invalid);
  TGNX_LAUNCH_CHECK("agg_count");
  if (dim == 0) return TGNX_OK;
  hipLaunchKernelGGL(agg_mean_bwd, dim3((unsigned)ceil_div(n_msg, WAVES)), dim3(OPS_BLOCK), 0, s, dout, index,
                     (const int*)cnt, n_msg, dim, dim_size, dmsg);
  TGNX_LAUNCH_CHECK("agg_mean_bwd");
  return TGNX_OK;
}

}  // extern "C"
