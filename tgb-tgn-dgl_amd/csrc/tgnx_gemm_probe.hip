// Test hooks over the MFMA GEMM core (tgnx_gemm.h): one GEMM on any of the tile configs the library compiles,
// direct or deferred split-K, with a grid cap, device-side runtime sizes and a gathered A operand; and one
// gemmN launch + one fixup launch hosting several jobs.  tests/test_gpu_gemm_core.py drives them; no product
// path calls them, and they add no kernel to any other entry point.
#include "tgnx_gemm.h"

using namespace tgnx;

namespace {

// Row-gathered row-major operand: element (r, k) at p[idx[r] * ld + k]; a two-phase loader (the index load,
// then the data loads) with the 16-B test of LoadRowK.  idx holds `rows` entries.
struct LoadGatherRowK {
  const float* p;
  const int64_t* idx;
  int rows, ks, ld;
  using Idx = int64_t;
  static constexpr bool row_idx = true;
  static constexpr bool k_fast = true;
  __device__ Idx index(int r, int) const { return idx[min(r, rows - 1)]; }
  __device__ float load(const Idx& i, int, int k) const { return p[i * ld + min(k, ks - 1)]; }
  __device__ bool vec4() const { return (ld & 3) == 0 && (ks & 3) == 0 && al16(p); }
  __device__ float4 load4(const Idx& i, int, int k) const {
    return *reinterpret_cast<const float4*>(p + i * ld + min(k, ks - 4));
  }
};

struct MarkBlock {  // a non-GEMM block: counts its own runs
  int* marks;
  __device__ void operator()(int bid, float*) const {
    if (threadIdx.x == 0) atomicAdd(&marks[bid], 1);
  }
};

// EpiStore that also notes which block of its grid finished each tile (who[base + capacity tile number])
struct EpiStoreWho {
  EpiStore st;
  int* who;
  int tiles_n, base;
  template <class T>
  __device__ void operator()(const T& t) const {
    st(t);
    if (who && threadIdx.x == 0) who[base + (t.m0 / T::tm) * tiles_n + t.n0 / T::tn] = blockIdx.x;
  }
};

template <class CFG>
GemmShape probe_shape(int smax, int grid_cap, int M, int N, int K, const int* Md, const int* Nd, const int* Kd) {
  GemmShape g = smax > 0 ? gemm_shape_split<CFG>(M, N, K, Md, Nd, Kd, smax) : gemm_shape<CFG>(M, N, K, Md, Nd, Kd);
  return grid_cap > 0 ? with_cap(g, grid_cap) : g;
}

// cfg -> f(CFG{}); false for an unknown cfg
template <class F>
bool with_cfg(int cfg, const F& f) {
  switch (cfg) {
    case TGNX_GEMM_PROBE_G32: f(G32{}); return true;
    case TGNX_GEMM_PROBE_G32L: f(G32L{}); return true;
    case TGNX_GEMM_PROBE_GW: f(GW{}); return true;
    case TGNX_GEMM_PROBE_G64: f(G64{}); return true;
    case TGNX_GEMM_PROBE_GD: f(GD{}); return true;
    default: return false;
  }
}

bool sizes_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 0 && N >= 0 && K >= 0 && M < (1 << 30) && N < (1 << 30) && K < (1 << 30);
}
size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

size_t tgnx_gemm_probe_ws_bytes(int32_t cfg, int32_t smax, int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || !sizes_ok(M, N, K)) return 256;
  size_t floats = 0;
  with_cfg(cfg, [&](auto c) {
    floats = gemm_partial_floats(probe_shape<decltype(c)>(smax, 0, (int)M, (int)N, (int)K, nullptr, nullptr, nullptr));
  });
  return floats * 4 + 256;
}

int tgnx_gemm_probe(int32_t cfg, int32_t smax, int32_t grid_cap, int64_t M, int64_t N, int64_t K,
                    const int32_t* dims_dev, const float* A, int64_t lda, int32_t trans_a, const int64_t* a_rows,
                    const float* B, int64_t ldb, int32_t trans_b, float* C, int64_t ldc, const float* bias,
                    int32_t accumulate, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(sizes_ok(M, N, K), "tgnx_gemm_probe: bad sizes");
  TGNX_CHECK_ARG(with_cfg(cfg, [](auto) {}), "tgnx_gemm_probe: unknown cfg %d", (int)cfg);
  TGNX_CHECK_ARG(smax >= 0 && smax <= 64 && grid_cap >= 0, "tgnx_gemm_probe: bad smax / grid_cap");
  TGNX_CHECK_ARG(!(a_rows && trans_a), "tgnx_gemm_probe: a_rows gathers rows of a row-major A (trans_a = 0)");
  if (M == 0 || N == 0) return TGNX_OK;
  TGNX_CHECK_ARG(K > 0, "tgnx_gemm_probe: K must be positive");
  TGNX_CHECK_ARG(A && B && C && ws, "tgnx_gemm_probe: null pointer");
  TGNX_CHECK_ARG(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N && lda < (1 << 30) &&
                     ldb < (1 << 30) && ldc < (1 << 30),
                 "tgnx_gemm_probe: leading dimension below the operand's width");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_gemm_probe_ws_bytes(cfg, smax, M, N, K), "tgnx_gemm_probe: workspace too small");
  hipStream_t s = as_stream(stream);
  const int *Md = nullptr, *Nd = nullptr, *Kd = nullptr;
  if (dims_dev) {  // which of the three are passed is the host's choice: read them back
    int32_t h[3];
    TGNX_HIP_CHECK(hipMemcpyAsync(h, dims_dev, sizeof(h), hipMemcpyDeviceToHost, s));
    TGNX_HIP_CHECK(hipStreamSynchronize(s));
    TGNX_CHECK_ARG(h[0] <= M && h[1] <= N && h[2] <= K, "tgnx_gemm_probe: runtime size above the capacity");
    if (h[0] >= 0) Md = dims_dev;
    if (h[1] >= 0) Nd = dims_dev + 1;
    if (h[2] >= 0) Kd = dims_dev + 2;
  }
  float* part = reinterpret_cast<float*>(ws);
  const int Mc = (int)M, Nc = (int)N, Kc = (int)K;
  const EpiStore epi{C, bias, (int)ldc, accumulate};
  auto run = [&](const auto& al, const auto& bl) {
    with_cfg(cfg, [&](auto c) {
      using CFG = decltype(c);
      const GemmShape g = probe_shape<CFG>(smax, grid_cap, Mc, Nc, Kc, Md, Nd, Kd);
      gemm_launch<CFG>(g, al, bl, epi, part, s);
      if (g.deferred) gemm_fixup_launch(0, NoTail{}, s, gemm_fix<CFG>(g, part, epi));
    });
  };
  auto with_b = [&](const auto& al) {
    if (trans_b) run(al, LoadRowK{B, Nc, Kc, (int)ldb});
    else run(al, LoadKRow{B, Nc, Kc, (int)ldb});
  };
  if (a_rows) with_b(LoadGatherRowK{A, a_rows, Mc, Kc, (int)lda});
  else if (!trans_a) with_b(LoadRowK{A, Mc, Kc, (int)lda});
  else with_b(LoadKRow{A, Mc, Kc, (int)lda});
  TGNX_LAUNCH_CHECK("tgnx_gemm_probe");
  return TGNX_OK;
}

// jobs[0]: G32 direct, C = A B^T; jobs[1]: GW deferred, C = A^T B; jobs[2]: GW deferred, C = A B^T
static GemmShape batch_shape(const tgnx_gemm_probe_job* jobs, int i) {
  const tgnx_gemm_probe_job& j = jobs[i];
  if (i == 0) return gemm_shape<G32>((int)j.M, (int)j.N, (int)j.K);
  return gemm_shape_split<GW>((int)j.M, (int)j.N, (int)j.K, nullptr, nullptr, nullptr, j.smax);
}

size_t tgnx_gemm_probe_batch_ws_bytes(const tgnx_gemm_probe_job* jobs) {
  if (!jobs) return 256;
  size_t b = 256;
  for (int i = 1; i < 3; ++i) {
    const tgnx_gemm_probe_job& j = jobs[i];
    if (j.M <= 0 || j.N <= 0 || j.K <= 0 || !sizes_ok(j.M, j.N, j.K) || j.smax < 1 || j.smax > 64) return 256;
    b += pad256(gemm_partial_floats(batch_shape(jobs, i)) * 4);
  }
  return b;
}

int tgnx_gemm_probe_batch(const tgnx_gemm_probe_job* jobs, int32_t nb, int32_t* marks, int32_t head,
                          int32_t tail_blocks, int32_t* tail_marks, int32_t* fix_blocks, void* ws, size_t ws_bytes,
                          void* stream) {
  TGNX_CHECK_ARG(jobs && ws, "tgnx_gemm_probe_batch: null pointer");
  for (int i = 0; i < 3; ++i) {
    const tgnx_gemm_probe_job& j = jobs[i];
    TGNX_CHECK_ARG(sizes_ok(j.M, j.N, j.K) && j.M > 0 && j.N > 0 && j.K > 0, "tgnx_gemm_probe_batch: bad sizes");
    TGNX_CHECK_ARG(j.A && j.B && j.C, "tgnx_gemm_probe_batch: null operand");
    const bool ta = i == 1, tb = i != 1;
    TGNX_CHECK_ARG(j.lda >= (ta ? j.M : j.K) && j.ldb >= (tb ? j.K : j.N) && j.ldc >= j.N && j.lda < (1 << 30) &&
                       j.ldb < (1 << 30) && j.ldc < (1 << 30),
                   "tgnx_gemm_probe_batch: leading dimension below the operand's width");
    TGNX_CHECK_ARG(i == 0 || (j.smax >= 1 && j.smax <= 64), "tgnx_gemm_probe_batch: bad smax");
  }
  TGNX_CHECK_ARG(nb >= 0 && nb < (1 << 20) && (nb == 0 || marks), "tgnx_gemm_probe_batch: bad nb / marks");
  // the first `head` of the tail_blocks tail blocks lead the fixup grid
  TGNX_CHECK_ARG(head >= 0 && head <= tail_blocks && tail_blocks < (1 << 20) && (tail_blocks == 0 || tail_marks),
                 "tgnx_gemm_probe_batch: head must lie in [0, tail_blocks]");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_gemm_probe_batch_ws_bytes(jobs), "tgnx_gemm_probe_batch: workspace too small");
  hipStream_t s = as_stream(stream);
  const GemmShape g0 = batch_shape(jobs, 0), g1 = batch_shape(jobs, 1), g2 = batch_shape(jobs, 2);
  float* p1 = reinterpret_cast<float*>(ws);
  float* p2 = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + pad256(gemm_partial_floats(g1) * 4));
  const tgnx_gemm_probe_job &j0 = jobs[0], &j1 = jobs[1], &j2 = jobs[2];
  const EpiStore e0{j0.C, j0.bias, (int)j0.ldc, j0.accumulate};
  const EpiStoreWho e1{EpiStore{j1.C, j1.bias, (int)j1.ldc, j1.accumulate}, fix_blocks, g1.tiles_n, 0},
      e2{EpiStore{j2.C, j2.bias, (int)j2.ldc, j2.accumulate}, fix_blocks, g2.tiles_n, g1.tiles_m * g1.tiles_n};
  gemmN_launch(s,
               gemm_job<G32>(g0, LoadRowK{j0.A, g0.M, g0.K, (int)j0.lda}, LoadRowK{j0.B, g0.N, g0.K, (int)j0.ldb}, e0,
                             nullptr),
               gemm_job<GW>(g1, LoadKRow{j1.A, g1.M, g1.K, (int)j1.lda}, LoadKRow{j1.B, g1.N, g1.K, (int)j1.ldb},
                            EpiDeferred{}, p1),
               gemm_job<GW>(g2, LoadRowK{j2.A, g2.M, g2.K, (int)j2.lda}, LoadRowK{j2.B, g2.N, g2.K, (int)j2.ldb},
                            EpiDeferred{}, p2),
               BlockJob<MarkBlock>{MarkBlock{marks}, nb});
  gemm_fixup_launch_h(head, tail_blocks, MarkBlock{tail_marks}, s, gemm_fix<GW>(g1, p1, e1), gemm_fix<GW>(g2, p2, e2));
  TGNX_LAUNCH_CHECK("tgnx_gemm_probe_batch");
  return TGNX_OK;
}

}  // extern "C"
