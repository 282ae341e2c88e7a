// torch.ops.tgnx — the C ABI of libtgnx (include/tgnx.h) registered as PyTorch operators (SURVEY §8b:
// "wrapped by TORCH_LIBRARY(tgnx, ...) ops").  Host code only: every op checks its tensors, allocates its
// outputs / workspace through PyTorch's caching allocator and calls the C entry point on the current HIP
// stream; errors raise RuntimeError with tgnx_last_error().  The fused TGN / TGNN steps keep their struct
// interface (tgnx_tgn_config / tgnx_tgn_buffers, driven by tgnx/tgn.py); these ops are the building blocks a
// torch caller composes directly:
//
//   ring_reset / ring_sample / ring_insert   LastNeighborLoader reset_state / __call__ / insert
//                                            (neighbor_loader.py:106-109, :26-50, :52-104); also registered under
//                                            SURVEY §8b's names reset / sample_recent / insert_recent
//   neg_sample                               NegLinkSamplerDest.sample (neg_sampler.py:8-23)
//   block_ids                                get_block / dependecyAwareBatch (dependencyGraph.py:8-49), CPU
//   tcsr_build / tcsr_sample                 TGL's ext_full.npz + recent sampler (utils.py:73, README.md:2-5)
//   pair_index_build / pair_index_contains / negs_hist_rnd
//                                            the (source, destination) pair index and TGB's hist_rnd evaluation
//                                            negatives drawn from it (csrc/tgnx_negs.hip; tgnx/tgb_negs.py)
//   pairset_insert / pairset_lookup / pairset_select
//                                            the live (source, destination) pair set (csrc/tgnx_pairset.hip;
//                                            tgnx/pairset.py allocates the table and applies the growth rule)
//   gemm_f32                                 the modules' Linear contractions on the MFMA GEMM
//   msg_agg_last / msg_agg_mean              LastAggregator / MeanAggregator (modules/msg_agg.py:15-26)
//   gru_update                               TGNMemory.memory_updater GRUCell / RNNCell (memory_module.py:70-78)
//   predictor                                LinkPredictor (decoder.py:12-27) / EdgePredictor (model_utils.py:165-195)
//   edge_attn_fwd / edge_attn_bwd            TransformerConv's attention (emb_module.py:21-29, PyG semantics)
//   edge_attn_drop_fwd / edge_attn_drop_bwd  the same with attention dropout under the engine's counter-based mask
//   time_encode / time_embedding             TimeEncoder ([ext] PyG) / TimeEmbedding (emb_module.py:32-52)
//   col_sum, gru_update_bwd, predictor_bwd, time_encode_bwd, time_embedding_bwd, msg_agg_last_bwd,
//   msg_agg_mean_bwd                         the backward halves (csrc/tgnx_ops_bwd.hip) behind tgnx/ops.py's
//                                            autograd functions
//   memstore_put / memstore_count / memstore_gather / memstore_build_msg
//                                            the device message store of tgnx.nn.TGNMemory / DyRepMemory
//                                            (memory_module.py:140-145, :180-207; csrc/tgnx_memstore.hip)
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <initializer_list>
#include <tuple>

#include "../../include/tgnx.h"

namespace {

// the current stream OF THE CURRENT DEVICE: every op first makes its tensors' device current (a device guard,
// restored on return), so the launch goes to that device's stream with that device's pointers
void* cur_stream() { return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream().stream()); }

// every device tensor of an op on one device (the one its guard selects)
void same_device(const at::Tensor& ref, std::initializer_list<const at::Tensor*> xs) {
  for (const at::Tensor* x : xs)
    TORCH_CHECK(x->device() == ref.device(), "tgnx: all tensors of an op must be on one device: ", ref.device(),
                " and ", x->device());
}

void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == TGNX_OK, what, " failed (", rc, "): ", tgnx_last_error());
}

void dev_tensor(const at::Tensor& x, at::ScalarType st, const char* name) {
  TORCH_CHECK(x.is_cuda(), name, " must be a HIP device tensor");
  TORCH_CHECK(x.scalar_type() == st, name, " has dtype ", x.scalar_type(), ", expected ", st);
  TORCH_CHECK(x.is_contiguous(), name, " must be contiguous");
}

void ring_state(const at::Tensor& nbr, const at::Tensor& eid, const at::Tensor& t) {
  dev_tensor(nbr, at::kLong, "nbr");
  dev_tensor(eid, at::kLong, "e_id");
  dev_tensor(t, at::kFloat, "t");
  TORCH_CHECK(nbr.dim() == 2 && eid.sizes() == nbr.sizes() && t.sizes() == nbr.sizes(),
              "ring tensors must be [num_nodes, size]");
}

void ring_reset(at::Tensor eid, at::Tensor t) {
  dev_tensor(eid, at::kLong, "e_id");
  dev_tensor(t, at::kFloat, "t");
  TORCH_CHECK(eid.dim() == 2 && t.sizes() == eid.sizes(), "ring tensors must be [num_nodes, size]");
  same_device(eid, {&t});
  const c10::OptionalDeviceGuard guard(eid.device());
  check_rc(tgnx_ring_reset(eid.data_ptr<int64_t>(), t.data_ptr<float>(), eid.size(0), (int32_t)eid.size(1),
                           cur_stream()),
           "tgnx_ring_reset");
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> ring_sample(const at::Tensor& nbr, const at::Tensor& eid,
                                                                       const at::Tensor& t, at::Tensor assoc,
                                                                       const at::Tensor& n_id) {
  ring_state(nbr, eid, t);
  dev_tensor(assoc, at::kLong, "assoc");
  dev_tensor(n_id, at::kLong, "n_id");
  same_device(nbr, {&eid, &t, &assoc, &n_id});
  const c10::OptionalDeviceGuard guard(nbr.device());
  const int64_t N = nbr.size(0), K = nbr.size(1), q = n_id.numel();
  TORCH_CHECK(assoc.numel() == N, "assoc must have num_nodes entries");
  const int64_t cap_n = std::max<int64_t>(q * (1 + K), 1), cap_e = std::max<int64_t>(q * K, 1);
  auto lopt = n_id.options();
  at::Tensor out_nid = at::empty({cap_n}, lopt), out_ei = at::empty({2 * cap_e}, lopt);
  at::Tensor out_eid = at::empty({cap_e}, lopt), out_t = at::empty({cap_e}, t.options());
  at::Tensor counts = at::zeros({2}, lopt);
  const size_t nb = tgnx_ring_sample_ws_bytes(N, q);
  at::Tensor ws = at::zeros({(int64_t)std::max<size_t>(nb, 1)}, n_id.options().dtype(at::kByte));
  check_rc(tgnx_ring_sample(nbr.data_ptr<int64_t>(), eid.data_ptr<int64_t>(), t.data_ptr<float>(), N, (int32_t)K,
                            n_id.data_ptr<int64_t>(), q, assoc.data_ptr<int64_t>(), out_nid.data_ptr<int64_t>(),
                            out_ei.data_ptr<int64_t>(), out_eid.data_ptr<int64_t>(), out_t.data_ptr<float>(), cap_n,
                            cap_e, counts.data_ptr<int64_t>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_ring_sample");
  const at::Tensor c = counts.cpu();  // one device -> host sync, as the reference's unique()
  const int64_t M = c.data_ptr<int64_t>()[0], E = c.data_ptr<int64_t>()[1];
  return {out_nid.narrow(0, 0, M), out_ei.view({2, cap_e}).narrow(1, 0, E), out_eid.narrow(0, 0, E),
          out_t.narrow(0, 0, E)};
}

void ring_insert(at::Tensor nbr, at::Tensor eid, at::Tensor t, const at::Tensor& src, const at::Tensor& dst,
                 const at::Tensor& ev_t, int64_t cur_e_id, at::Tensor assoc) {
  ring_state(nbr, eid, t);
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  dev_tensor(ev_t, at::kFloat, "ev_t");
  dev_tensor(assoc, at::kLong, "assoc");
  same_device(nbr, {&eid, &t, &src, &dst, &ev_t, &assoc});
  const c10::OptionalDeviceGuard guard(nbr.device());
  const int64_t B = src.numel();
  TORCH_CHECK(dst.numel() == B && ev_t.numel() == B, "src, dst, ev_t must have the same length");
  TORCH_CHECK(B <= tgnx_ring_insert_max_batch(), "batch ", B, " > ", tgnx_ring_insert_max_batch());
  check_rc(tgnx_ring_insert(nbr.data_ptr<int64_t>(), eid.data_ptr<int64_t>(), t.data_ptr<float>(), nbr.size(0),
                            (int32_t)nbr.size(1), src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(),
                            ev_t.data_ptr<float>(), B, cur_e_id, assoc.data_ptr<int64_t>(), cur_stream()),
           "tgnx_ring_insert");
}

at::Tensor neg_sample(const at::Tensor& dst_nodes, const at::Tensor& pos, int64_t seed, int64_t offset) {
  dev_tensor(dst_nodes, at::kLong, "dst_nodes");
  dev_tensor(pos, at::kLong, "pos");
  TORCH_CHECK(dst_nodes.numel() > 0, "empty destination set");
  same_device(dst_nodes, {&pos});
  const c10::OptionalDeviceGuard guard(dst_nodes.device());
  at::Tensor out = at::empty_like(pos);
  check_rc(tgnx_neg_sample(dst_nodes.data_ptr<int64_t>(), dst_nodes.numel(), pos.data_ptr<int64_t>(), pos.numel(),
                           (uint64_t)seed, (uint64_t)offset, out.data_ptr<int64_t>(), cur_stream()),
           "tgnx_neg_sample");
  return out;
}

at::Tensor block_ids(const at::Tensor& src, const at::Tensor& dst, int64_t batch) {
  TORCH_CHECK(!src.is_cuda() && !dst.is_cuda(), "block_ids runs on host tensors (dependencyGraph.py is CPU code)");
  const at::Tensor s = src.to(at::kLong).contiguous(), d = dst.to(at::kLong).contiguous();
  TORCH_CHECK(s.numel() == d.numel(), "src and dst must have the same length");
  at::Tensor out = at::empty_like(s);
  check_rc(tgnx_block_ids_host(s.data_ptr<int64_t>(), d.data_ptr<int64_t>(), s.numel(), batch,
                               out.data_ptr<int64_t>()),
           "tgnx_block_ids_host");
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, bool> tcsr_build(const at::Tensor& src,
                                                                             const at::Tensor& dst,
                                                                             const at::Tensor& t, int64_t num_nodes,
                                                                             bool add_reverse) {
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  dev_tensor(t, at::kFloat, "t");
  same_device(src, {&dst, &t});
  const c10::OptionalDeviceGuard guard(src.device());
  const int64_t E = src.numel(), nnz = add_reverse ? 2 * E : E;
  auto lopt = src.options();
  at::Tensor indptr = at::empty({num_nodes + 1}, lopt), indices = at::empty({std::max<int64_t>(nnz, 1)}, lopt);
  at::Tensor eid = at::empty({std::max<int64_t>(nnz, 1)}, lopt), ts = at::empty({std::max<int64_t>(nnz, 1)}, t.options());
  at::Tensor chrono = at::zeros({1}, lopt.dtype(at::kInt));
  const size_t nb = tgnx_tcsr_build_ws_bytes(E, add_reverse ? 1 : 0);
  at::Tensor ws = at::empty({(int64_t)std::max<size_t>(nb, 1)}, lopt.dtype(at::kByte));
  check_rc(tgnx_tcsr_build(src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), t.data_ptr<float>(), E, num_nodes,
                           add_reverse ? 1 : 0, indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(),
                           eid.data_ptr<int64_t>(), ts.data_ptr<float>(), chrono.data_ptr<int32_t>(), ws.data_ptr(), nb,
                           cur_stream()),
           "tgnx_tcsr_build");
  const bool chr = chrono.cpu().data_ptr<int32_t>()[0] != 0;
  return {indptr, indices.narrow(0, 0, nnz), eid.narrow(0, 0, nnz), ts.narrow(0, 0, nnz), chr};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> tcsr_sample(const at::Tensor& indptr,
                                                                       const at::Tensor& indices,
                                                                       const at::Tensor& eid, const at::Tensor& ts,
                                                                       int64_t K, const at::Tensor& roots,
                                                                       int64_t mode, const at::Tensor& cut) {
  dev_tensor(indptr, at::kLong, "indptr");
  dev_tensor(indices, at::kLong, "indices");
  dev_tensor(eid, at::kLong, "eid");
  dev_tensor(ts, at::kFloat, "ts");
  dev_tensor(roots, at::kLong, "roots");
  TORCH_CHECK(mode == 0 || mode == 1, "mode 0 (event-id cutoff) or 1 (time cutoff)");
  dev_tensor(cut, mode == 0 ? at::kLong : at::kFloat, "cut");
  same_device(indptr, {&indices, &eid, &ts, &roots, &cut});
  const c10::OptionalDeviceGuard guard(indptr.device());
  const int64_t Q = roots.numel();
  TORCH_CHECK(cut.numel() == Q, "one cutoff per root");
  auto lopt = roots.options();
  at::Tensor nbr = at::empty({Q, K}, lopt), oe = at::empty({Q, K}, lopt), ot = at::empty({Q, K}, ts.options());
  at::Tensor cnt = at::empty({Q}, lopt.dtype(at::kInt));
  check_rc(tgnx_tcsr_sample(indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), eid.data_ptr<int64_t>(),
                            ts.data_ptr<float>(), indptr.numel() - 1, (int32_t)K, roots.data_ptr<int64_t>(), Q,
                            (int32_t)mode, mode == 0 ? cut.data_ptr<int64_t>() : nullptr, 0,
                            mode == 1 ? cut.data_ptr<float>() : nullptr, nbr.data_ptr<int64_t>(), oe.data_ptr<int64_t>(),
                            ot.data_ptr<float>(), cnt.data_ptr<int32_t>(), cur_stream()),
           "tgnx_tcsr_sample");
  return {nbr, oe, ot, cnt};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> pair_index_build(const at::Tensor& src, const at::Tensor& dst,
                                                                int64_t num_nodes) {
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  same_device(src, {&dst});
  TORCH_CHECK(dst.numel() == src.numel(), "src and dst must have the same length");
  const c10::OptionalDeviceGuard guard(src.device());
  const int64_t n = src.numel();
  auto lopt = src.options();
  at::Tensor indptr = at::empty({num_nodes + 1}, lopt), indices = at::empty({std::max<int64_t>(n, 1)}, lopt);
  at::Tensor first = at::empty({std::max<int64_t>(n, 1)}, lopt);
  const size_t nb = tgnx_pair_index_build_ws_bytes(n);
  at::Tensor ws = at::empty({(int64_t)std::max<size_t>(nb, 1)}, lopt.dtype(at::kByte));
  int64_t nnz = 0;
  check_rc(tgnx_pair_index_build(src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), n, num_nodes,
                                 indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), first.data_ptr<int64_t>(), &nnz,
                                 ws.data_ptr(), nb, cur_stream()),
           "tgnx_pair_index_build");
  return {indptr, indices.narrow(0, 0, nnz), first.narrow(0, 0, nnz)};
}

at::Tensor pair_index_contains(const at::Tensor& indptr, const at::Tensor& indices, const at::Tensor& first,
                               const at::Tensor& src, const at::Tensor& dst, const c10::optional<at::Tensor>& before,
                               int64_t before_all) {
  dev_tensor(indptr, at::kLong, "indptr");
  dev_tensor(indices, at::kLong, "indices");
  dev_tensor(first, at::kLong, "first");
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  same_device(indptr, {&indices, &first, &src, &dst});
  const int64_t n = src.numel();
  TORCH_CHECK(dst.numel() == n && first.numel() == indices.numel() && indptr.numel() >= 2, "pair_index_contains: shapes");
  const int64_t* pb = nullptr;
  if (before.has_value()) {
    dev_tensor(*before, at::kLong, "before");
    same_device(indptr, {&*before});
    TORCH_CHECK(before->numel() == n, "one row cut per query");
    pb = before->data_ptr<int64_t>();
  }
  const c10::OptionalDeviceGuard guard(indptr.device());
  at::Tensor out = at::empty({n}, src.options().dtype(at::kBool));
  check_rc(tgnx_pair_index_contains(indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), first.data_ptr<int64_t>(),
                                    indptr.numel() - 1, src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), n, pb,
                                    before_all, reinterpret_cast<uint8_t*>(out.data_ptr<bool>()), cur_stream()),
           "tgnx_pair_index_contains");
  return out;
}

// (rows [hi - lo, k], k_hist int32[hi - lo], status int64[4] on the device: the caller reads it)
std::tuple<at::Tensor, at::Tensor, at::Tensor> negs_hist_rnd(const at::Tensor& src, const at::Tensor& dst,
                                                             const at::Tensor& t, int64_t lo, int64_t hi, int64_t k,
                                                             int64_t q, int64_t hist_hi, const at::Tensor& indptr,
                                                             const at::Tensor& indices, const at::Tensor& first,
                                                             const at::Tensor& pool, int64_t seed, int64_t max_draws) {
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  TORCH_CHECK(t.scalar_type() == at::kDouble || t.scalar_type() == at::kFloat, "t must be float64 or float32");
  dev_tensor(t, t.scalar_type(), "t");
  dev_tensor(indptr, at::kLong, "indptr");
  dev_tensor(indices, at::kLong, "indices");
  dev_tensor(first, at::kLong, "first");
  dev_tensor(pool, at::kLong, "pool");
  same_device(src, {&dst, &t, &indptr, &indices, &first, &pool});
  const int64_t E = src.numel();
  TORCH_CHECK(dst.numel() == E && t.numel() == E && first.numel() == indices.numel() && indptr.numel() >= 2,
              "negs_hist_rnd: shapes");
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= E, "rows [lo, hi) outside the event table");
  TORCH_CHECK(k >= 1 && k <= 1024 && q >= 0 && q <= k, "negs_hist_rnd: k must be in [1, 1024] and q in [0, k]");
  const c10::OptionalDeviceGuard guard(src.device());
  auto lopt = src.options();
  at::Tensor out = at::empty({hi - lo, k}, lopt), k_hist = at::empty({hi - lo}, lopt.dtype(at::kInt));
  at::Tensor status = at::empty({4}, lopt);
  const size_t nb = tgnx_negs_hist_rnd_ws_bytes(indices.numel(), hi - lo);
  at::Tensor ws = at::empty({(int64_t)std::max<size_t>(nb, 1)}, lopt.dtype(at::kByte));
  check_rc(tgnx_negs_hist_rnd(src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), t.data_ptr(),
                              t.scalar_type() == at::kDouble ? 1 : 0, E, lo, hi, (int32_t)k, (int32_t)q, hist_hi,
                              indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), first.data_ptr<int64_t>(),
                              indptr.numel() - 1, indices.numel(), pool.data_ptr<int64_t>(), pool.numel(), (uint64_t)seed,
                              max_draws, out.data_ptr<int64_t>(), k_hist.data_ptr<int32_t>(), status.data_ptr<int64_t>(),
                              ws.data_ptr(), nb, cur_stream()),
           "tgnx_negs_hist_rnd");
  return {out, k_hist, status};
}

// ---- live pair set (csrc/tgnx_pairset.hip; tgnx/pairset.py owns allocation and the growth rule).  table is the
// int64 view of a tgnx_pairset_bytes(capacity) allocation: capacity = numel * 2 / 5.
int64_t pairset_capacity(const at::Tensor& table) {
  dev_tensor(table, at::kLong, "table");
  const int64_t cap = table.numel() * 2 / 5;
  TORCH_CHECK(cap >= 64 && (cap & (cap - 1)) == 0 && tgnx_pairset_bytes(cap) == (size_t)table.numel() * 8,
              "table must be the int64 view of a pair set of a power-of-two capacity >= 64");
  return cap;
}

const float* pairset_since(const at::Tensor& table, const c10::optional<at::Tensor>& since, int64_t n) {
  if (!since.has_value()) return nullptr;
  dev_tensor(*since, at::kFloat, "since");
  same_device(table, {&*since});
  TORCH_CHECK(since->numel() == n, "one cut per query");
  return since->data_ptr<float>();
}

// The op checks the chunk size only.  The caller owns the growth rule (tgnx/pairset.py: read status[0] on schedule,
// rehash into a larger table before the load passes 1/2): an insert into a table that is too full does not fail, it
// counts the events it had no slot for in status[2].
void pairset_insert(at::Tensor table, at::Tensor status, const at::Tensor& src, const at::Tensor& dst,
                    const at::Tensor& t, int64_t num_nodes) {
  const int64_t cap = pairset_capacity(table);
  dev_tensor(status, at::kLong, "status");
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  dev_tensor(t, at::kFloat, "t");
  same_device(table, {&status, &src, &dst, &t});
  const int64_t n = src.numel();
  TORCH_CHECK(dst.numel() == n && t.numel() == n && status.numel() >= 3, "pairset_insert: shapes");
  TORCH_CHECK(n <= cap / 8, "pairset_insert: at most capacity / 8 events per call (the growth rule's chunk)");
  const c10::OptionalDeviceGuard guard(table.device());
  check_rc(tgnx_pairset_insert(table.data_ptr(), cap, src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(),
                               t.data_ptr<float>(), n, num_nodes, status.data_ptr<int64_t>(), cur_stream()),
           "tgnx_pairset_insert");
}

// (seen bool[n], count int64[n], t_first float32[n], t_last float32[n])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> pairset_lookup(const at::Tensor& table, const at::Tensor& src,
                                                                          const at::Tensor& dst, int64_t num_nodes,
                                                                          const c10::optional<at::Tensor>& since,
                                                                          c10::optional<double> since_all) {
  const int64_t cap = pairset_capacity(table);
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  same_device(table, {&src, &dst});
  const int64_t n = src.numel();
  TORCH_CHECK(dst.numel() == n, "pairset_lookup: shapes");
  const float* ps = pairset_since(table, since, n);
  const c10::OptionalDeviceGuard guard(table.device());
  at::Tensor seen = at::empty({n}, src.options().dtype(at::kBool)), count = at::empty({n}, src.options());
  at::Tensor tf = at::empty({n}, src.options().dtype(at::kFloat)), tl = at::empty({n}, src.options().dtype(at::kFloat));
  check_rc(tgnx_pairset_lookup(table.data_ptr(), cap, num_nodes, src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), n, ps,
                               since_all.has_value() ? (float)*since_all : -INFINITY,
                               reinterpret_cast<uint8_t*>(seen.data_ptr<bool>()), count.data_ptr<int64_t>(),
                               tf.data_ptr<float>(), tl.data_ptr<float>(), cur_stream()),
           "tgnx_pairset_lookup");
  return {seen, count, tf, tl};
}

// (ptr int64[Q + 1], ids): one host read of ptr[Q] sizes the ids
std::tuple<at::Tensor, at::Tensor> pairset_select(const at::Tensor& table, const at::Tensor& src, const at::Tensor& cand,
                                                  int64_t num_nodes, const c10::optional<at::Tensor>& since,
                                                  c10::optional<double> since_all) {
  const int64_t cap = pairset_capacity(table);
  dev_tensor(src, at::kLong, "src");
  dev_tensor(cand, at::kLong, "cand");
  same_device(table, {&src, &cand});
  const int64_t Q = src.numel(), C = cand.numel();
  const float* ps = pairset_since(table, since, Q);
  const float cut = since_all.has_value() ? (float)*since_all : -INFINITY;
  const c10::OptionalDeviceGuard guard(table.device());
  const size_t nb = tgnx_pairset_select_ws_bytes(Q, C);
  TORCH_CHECK(nb > 0, "pairset_select: Q x C beyond one call");
  at::Tensor ws = at::empty({(int64_t)nb}, src.options().dtype(at::kByte));
  at::Tensor ptr = at::empty({Q + 1}, src.options());
  check_rc(tgnx_pairset_select_count(table.data_ptr(), cap, num_nodes, src.data_ptr<int64_t>(), Q,
                                     cand.data_ptr<int64_t>(), C, ps, cut, ptr.data_ptr<int64_t>(), ws.data_ptr(), nb,
                                     cur_stream()),
           "tgnx_pairset_select_count");
  const int64_t total = ptr[Q].item<int64_t>();
  at::Tensor ids = at::empty({total}, src.options());
  check_rc(tgnx_pairset_select_fill(table.data_ptr(), cap, num_nodes, src.data_ptr<int64_t>(), Q,
                                    cand.data_ptr<int64_t>(), C, ps, cut, ids.data_ptr<int64_t>(), total, ws.data_ptr(),
                                    nb, cur_stream()),
           "tgnx_pairset_select_fill");
  return {ptr, ids};
}

at::Tensor gemm_f32(const at::Tensor& A, const at::Tensor& B, const c10::optional<at::Tensor>& bias, bool trans_a,
                    bool trans_b) {
  dev_tensor(A, at::kFloat, "A");
  dev_tensor(B, at::kFloat, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "A and B must be 2-D");
  same_device(A, {&B});
  const c10::OptionalDeviceGuard guard(A.device());
  const int64_t M = trans_a ? A.size(1) : A.size(0), K = trans_a ? A.size(0) : A.size(1);
  const int64_t KB = trans_b ? B.size(1) : B.size(0), N = trans_b ? B.size(0) : B.size(1);
  TORCH_CHECK(K == KB, "inner dimensions differ: ", K, " vs ", KB);
  const float* bp = nullptr;
  if (bias.has_value()) {
    dev_tensor(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == N, "bias must have N entries");
    same_device(A, {&*bias});
    bp = bias->data_ptr<float>();
  }
  at::Tensor C = at::empty({M, N}, A.options());
  const size_t nb = tgnx_gemm_f32_ws_bytes(M, N, K);
  at::Tensor ws = at::empty({(int64_t)nb}, A.options().dtype(at::kByte));
  check_rc(tgnx_gemm_f32(M, N, K, A.data_ptr<float>(), A.size(1), trans_a ? 1 : 0, B.data_ptr<float>(), B.size(1),
                         trans_b ? 1 : 0, C.data_ptr<float>(), N, bp, 0, ws.data_ptr(), nb, cur_stream()),
           "tgnx_gemm_f32");
  return C;
}

const float* opt_ptr(const c10::optional<at::Tensor>& x, const at::Tensor& ref, int64_t numel, const char* name) {
  if (!x.has_value()) return nullptr;
  dev_tensor(*x, at::kFloat, name);
  TORCH_CHECK(x->numel() == numel, name, " must have ", numel, " entries");
  same_device(ref, {&*x});
  return x->data_ptr<float>();
}

// out-of-range index -> RuntimeError, as the reference's scatter (one device -> host read of the drop count)
std::tuple<at::Tensor, at::Tensor> msg_agg(int32_t mode, const at::Tensor& msg, const at::Tensor& index,
                                           const at::Tensor* t, int64_t dim_size) {
  dev_tensor(msg, at::kFloat, "msg");
  dev_tensor(index, at::kLong, "index");
  TORCH_CHECK(msg.dim() == 2, "msg must be [n_msg, dim]");
  TORCH_CHECK(index.dim() == 1 && index.numel() == msg.size(0), "index must be [n_msg]");
  TORCH_CHECK(dim_size >= 0, "dim_size must be non-negative");
  int32_t t_dtype = 0;
  if (t) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->numel() == msg.size(0), "t must be a contiguous [n_msg] device tensor");
    TORCH_CHECK(t->scalar_type() == at::kLong || t->scalar_type() == at::kFloat, "t must be int64 or float32");
    t_dtype = t->scalar_type() == at::kLong ? 0 : 1;
    same_device(msg, {t});
  }
  same_device(msg, {&index});
  const c10::OptionalDeviceGuard guard(msg.device());
  const int64_t n = msg.size(0), dim = msg.size(1);
  at::Tensor out = at::empty({dim_size, dim}, msg.options());
  at::Tensor arg = at::empty({dim_size}, index.options());
  at::Tensor bad = at::zeros({1}, index.options());
  const size_t nb = tgnx_msg_agg_ws_bytes(n, dim_size);
  at::Tensor ws = at::empty({(int64_t)std::max<size_t>(nb, 1)}, index.options().dtype(at::kByte));
  check_rc(tgnx_msg_agg(mode, msg.data_ptr<float>(), n, dim, index.data_ptr<int64_t>(), t ? t->data_ptr() : nullptr,
                        t_dtype, dim_size, out.data_ptr<float>(), arg.data_ptr<int64_t>(), bad.data_ptr<int64_t>(),
                        ws.data_ptr(), nb, cur_stream()),
           "tgnx_msg_agg");
  const int64_t nbad = bad.cpu().data_ptr<int64_t>()[0];
  TORCH_CHECK(nbad == 0, "msg_agg: ", nbad, " index entries outside [0, ", dim_size, ")");
  return {out, arg};
}

std::tuple<at::Tensor, at::Tensor> msg_agg_last(const at::Tensor& msg, const at::Tensor& index, const at::Tensor& t,
                                                int64_t dim_size) {
  return msg_agg(0, msg, index, &t, dim_size);
}

at::Tensor msg_agg_mean(const at::Tensor& msg, const at::Tensor& index, int64_t dim_size) {
  return std::get<0>(msg_agg(1, msg, index, nullptr, dim_size));
}

at::Tensor gru_update(const at::Tensor& x, const at::Tensor& h, const at::Tensor& w_ih, const at::Tensor& w_hh,
                      const c10::optional<at::Tensor>& b_ih, const c10::optional<at::Tensor>& b_hh, int64_t cell) {
  dev_tensor(x, at::kFloat, "x");
  dev_tensor(h, at::kFloat, "h");
  dev_tensor(w_ih, at::kFloat, "w_ih");
  dev_tensor(w_hh, at::kFloat, "w_hh");
  TORCH_CHECK(cell == 0 || cell == 1, "cell 0 (GRUCell) or 1 (RNNCell, tanh)");
  TORCH_CHECK(x.dim() == 2 && h.dim() == 2 && x.size(0) == h.size(0), "x [M, d_in] and h [M, D]");
  const int64_t M = x.size(0), d_in = x.size(1), D = h.size(1), G = (cell == 0 ? 3 : 1) * D;
  TORCH_CHECK(w_ih.dim() == 2 && w_ih.size(0) == G && w_ih.size(1) == d_in, "w_ih must be [", G, ", ", d_in, "]");
  TORCH_CHECK(w_hh.dim() == 2 && w_hh.size(0) == G && w_hh.size(1) == D, "w_hh must be [", G, ", ", D, "]");
  same_device(x, {&h, &w_ih, &w_hh});
  const float* bi = opt_ptr(b_ih, x, G, "b_ih");
  const float* bh = opt_ptr(b_hh, x, G, "b_hh");
  const c10::OptionalDeviceGuard guard(x.device());
  at::Tensor out = at::empty_like(h);
  const size_t nb = tgnx_memory_cell_ws_bytes(M, d_in, D);
  at::Tensor ws = at::empty({(int64_t)nb}, x.options().dtype(at::kByte));
  check_rc(tgnx_memory_cell((int32_t)cell, M, d_in, D, x.data_ptr<float>(), h.data_ptr<float>(), w_ih.data_ptr<float>(),
                            w_hh.data_ptr<float>(), bi, bh, out.data_ptr<float>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_memory_cell");
  return out;
}

at::Tensor predictor(const at::Tensor& z_src, const at::Tensor& z_dst, const at::Tensor& w_src,
                     const c10::optional<at::Tensor>& b_src, const at::Tensor& w_dst,
                     const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out,
                     bool sigmoid) {
  dev_tensor(z_src, at::kFloat, "z_src");
  dev_tensor(z_dst, at::kFloat, "z_dst");
  dev_tensor(w_src, at::kFloat, "w_src");
  dev_tensor(w_dst, at::kFloat, "w_dst");
  dev_tensor(w_out, at::kFloat, "w_out");
  dev_tensor(b_out, at::kFloat, "b_out");
  TORCH_CHECK(z_src.dim() == 2 && z_dst.dim() == 2 && z_src.size(1) == z_dst.size(1), "z_src [B, d] and z_dst [M, d]");
  const int64_t B = z_src.size(0), M = z_dst.size(0), d_in = z_src.size(1), D = w_src.size(0);
  TORCH_CHECK(M == 0 || (B > 0 && M % B == 0), "z_dst rows must be a multiple of z_src rows (tile pairing)");
  TORCH_CHECK(w_src.dim() == 2 && w_src.size(1) == d_in && w_dst.dim() == 2 && w_dst.size(0) == D &&
                  w_dst.size(1) == d_in,
              "w_src / w_dst must be [D, d]");
  TORCH_CHECK(w_out.numel() == D && b_out.numel() == 1, "w_out must have D entries and b_out one");
  same_device(z_src, {&z_dst, &w_src, &w_dst, &w_out, &b_out});
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  const c10::OptionalDeviceGuard guard(z_src.device());
  at::Tensor out = at::empty({M, 1}, z_src.options());
  const size_t nb = tgnx_link_predictor_ws_bytes(B, M, d_in, D);
  at::Tensor ws = at::empty({(int64_t)nb}, z_src.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor(B, M, d_in, D, z_src.data_ptr<float>(), z_dst.data_ptr<float>(), w_src.data_ptr<float>(),
                               bs, w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(), b_out.data_ptr<float>(),
                               sigmoid ? 1 : 0, out.data_ptr<float>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_link_predictor");
  return out;
}

// the argument checks of the top-k and rank ops (csrc/tgnx_topk.hip); returns (d_in, D)
std::pair<int64_t, int64_t> topk_args(const at::Tensor& z_src, const at::Tensor& z_cand, const at::Tensor& w_src,
                                      const at::Tensor& w_dst, const at::Tensor& w_out, const at::Tensor& b_out,
                                      int64_t k) {
  dev_tensor(z_src, at::kFloat, "z_src");
  dev_tensor(z_cand, at::kFloat, "z_cand");
  dev_tensor(w_src, at::kFloat, "w_src");
  dev_tensor(w_dst, at::kFloat, "w_dst");
  dev_tensor(w_out, at::kFloat, "w_out");
  dev_tensor(b_out, at::kFloat, "b_out");
  TORCH_CHECK(z_src.dim() == 2 && z_cand.dim() == 2 && z_src.size(1) == z_cand.size(1), "z_src [B, d] and z_cand [C, d]");
  const int64_t d_in = z_src.size(1), D = w_src.size(0);
  TORCH_CHECK(w_src.dim() == 2 && w_src.size(1) == d_in && w_dst.dim() == 2 && w_dst.size(0) == D &&
                  w_dst.size(1) == d_in,
              "w_src / w_dst must be [D, d]");
  TORCH_CHECK(w_out.numel() == D && b_out.numel() == 1, "w_out must have D entries and b_out one");
  TORCH_CHECK(k >= 1 && k <= TGNX_TOPK_MAX, "k must be in [1, ", TGNX_TOPK_MAX, "], got ", k);
  same_device(z_src, {&z_cand, &w_src, &w_dst, &w_out, &b_out});
  return {d_in, D};
}

// the dense ops' outputs: (val [B, k], idx [B, k], logits [B, C] or an empty tensor)
std::tuple<at::Tensor, at::Tensor, at::Tensor> topk_outputs(const at::Tensor& z_src, int64_t C, int64_t k,
                                                            bool return_scores) {
  const int64_t B = z_src.size(0);
  return {at::empty({B, k}, z_src.options()), at::empty({B, k}, z_src.options().dtype(at::kLong)),
          return_scores ? at::empty({B, C}, z_src.options()) : at::empty({0}, z_src.options())};
}

const int64_t* opt_long(const c10::optional<at::Tensor>& x, const at::Tensor& ref, int64_t numel, const char* name) {
  if (!x.has_value()) return nullptr;
  dev_tensor(*x, at::kLong, name);
  TORCH_CHECK(numel < 0 || x->numel() == numel, name, " must have ", numel, " entries");
  same_device(ref, {&*x});
  return x->data_ptr<int64_t>();
}

// the exclusion-by-key arguments of the filtered top-k and the rank op, checked: the C ABI's four pointers and nnz
struct KeyArgs {
  const int64_t *cand_key, *src_key, *excl_ptr, *excl_key;
  int64_t nnz;
};
KeyArgs key_args(const at::Tensor& z_src, int64_t C, const c10::optional<at::Tensor>& cand_key,
                 const c10::optional<at::Tensor>& src_key, const c10::optional<at::Tensor>& excl_ptr,
                 const c10::optional<at::Tensor>& excl_key) {
  const int64_t B = z_src.size(0);
  const KeyArgs a{opt_long(cand_key, z_src, C, "cand_key"), opt_long(src_key, z_src, B, "src_key"),  // (in this order)
                  opt_long(excl_ptr, z_src, B + 1, "excl_ptr"), opt_long(excl_key, z_src, -1, "excl_key"),
                  excl_key.has_value() ? excl_key->numel() : 0};
  TORCH_CHECK(!a.excl_ptr || excl_key.has_value(), "excl_ptr needs excl_key");
  return a;
}

// LinkPredictor over all (source, candidate) pairs with the top-k selection fused in (csrc/tgnx_topk.hip):
// (val [B, k], idx [B, k] positions into z_cand, logits [B, C] or an empty tensor)
std::tuple<at::Tensor, at::Tensor, at::Tensor> predictor_topk(
    const at::Tensor& z_src, const at::Tensor& z_cand, const at::Tensor& w_src, const c10::optional<at::Tensor>& b_src,
    const at::Tensor& w_dst, const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out,
    int64_t k, bool sigmoid, bool return_scores) {
  const auto [d_in, D] = topk_args(z_src, z_cand, w_src, w_dst, w_out, b_out, k);
  const int64_t B = z_src.size(0), C = z_cand.size(0);
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  const c10::OptionalDeviceGuard guard(z_src.device());
  auto [val, idx, all] = topk_outputs(z_src, C, k, return_scores);
  const size_t nb = tgnx_link_predictor_topk_ws_bytes(B, C, d_in, D, (int32_t)k);
  at::Tensor ws = at::empty({(int64_t)nb}, z_src.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor_topk(B, C, d_in, D, z_src.data_ptr<float>(), z_cand.data_ptr<float>(),
                                    w_src.data_ptr<float>(), bs, w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(),
                                    b_out.data_ptr<float>(), (int32_t)k, sigmoid ? 1 : 0, val.data_ptr<float>(),
                                    idx.data_ptr<int64_t>(), return_scores ? all.data_ptr<float>() : nullptr,
                                    ws.data_ptr(), nb, cur_stream()),
           "tgnx_link_predictor_topk");
  return {val, idx, all};
}

// predictor_topk with per-source exclusions by key (tgnx_link_predictor_topk_filtered); the logits are unmasked
std::tuple<at::Tensor, at::Tensor, at::Tensor> predictor_topk_filtered(
    const at::Tensor& z_src, const at::Tensor& z_cand, const at::Tensor& w_src, const c10::optional<at::Tensor>& b_src,
    const at::Tensor& w_dst, const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out,
    int64_t k, bool sigmoid, bool return_scores, const c10::optional<at::Tensor>& cand_key,
    const c10::optional<at::Tensor>& src_key, const c10::optional<at::Tensor>& excl_ptr,
    const c10::optional<at::Tensor>& excl_key) {
  const auto [d_in, D] = topk_args(z_src, z_cand, w_src, w_dst, w_out, b_out, k);
  const int64_t B = z_src.size(0), C = z_cand.size(0);
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  const KeyArgs f = key_args(z_src, C, cand_key, src_key, excl_ptr, excl_key);
  const c10::OptionalDeviceGuard guard(z_src.device());
  auto [val, idx, all] = topk_outputs(z_src, C, k, return_scores);
  const size_t nb = tgnx_link_predictor_topk_filtered_ws_bytes(B, C, d_in, D, (int32_t)k);
  at::Tensor ws = at::empty({(int64_t)nb}, z_src.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor_topk_filtered(
               B, C, d_in, D, z_src.data_ptr<float>(), z_cand.data_ptr<float>(), w_src.data_ptr<float>(), bs,
               w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(), b_out.data_ptr<float>(), (int32_t)k,
               sigmoid ? 1 : 0, f.cand_key, f.src_key, f.excl_ptr, f.excl_key, f.nnz, val.data_ptr<float>(),
               idx.data_ptr<int64_t>(), return_scores ? all.data_ptr<float>() : nullptr, ws.data_ptr(), nb,
               cur_stream()),
           "tgnx_link_predictor_topk_filtered");
  return {val, idx, all};
}

// nearest neighbours in embedding space with the top-k selection fused in (tgnx_embed_knn, csrc/tgnx_knn.hip):
// (val [Q, k], idx [Q, k] positions into z_cand, scores [Q, C] unmasked or an empty tensor)
std::tuple<at::Tensor, at::Tensor, at::Tensor> embed_knn(const at::Tensor& z_q, const at::Tensor& z_cand, int64_t metric,
                                                         int64_t k, bool return_scores,
                                                         const c10::optional<at::Tensor>& cand_key,
                                                         const c10::optional<at::Tensor>& q_key,
                                                         const c10::optional<at::Tensor>& excl_ptr,
                                                         const c10::optional<at::Tensor>& excl_key) {
  dev_tensor(z_q, at::kFloat, "z_q");
  dev_tensor(z_cand, at::kFloat, "z_cand");
  TORCH_CHECK(z_q.dim() == 2 && z_cand.dim() == 2 && z_q.size(1) == z_cand.size(1), "z_q [Q, D] and z_cand [C, D]");
  TORCH_CHECK(k >= 1 && k <= TGNX_TOPK_MAX, "k must be in [1, ", TGNX_TOPK_MAX, "], got ", k);
  TORCH_CHECK(metric == TGNX_KNN_DOT || metric == TGNX_KNN_COSINE, "metric must be 0 (dot) or 1 (cosine), got ", metric);
  same_device(z_q, {&z_cand});
  const int64_t Q = z_q.size(0), C = z_cand.size(0), D = z_q.size(1);
  const KeyArgs f = key_args(z_q, C, cand_key, q_key, excl_ptr, excl_key);
  const c10::OptionalDeviceGuard guard(z_q.device());
  auto [val, idx, all] = topk_outputs(z_q, C, k, return_scores);
  const size_t nb = tgnx_embed_knn_ws_bytes(Q, C, D, (int32_t)k);
  at::Tensor ws = at::empty({(int64_t)nb}, z_q.options().dtype(at::kByte));
  check_rc(tgnx_embed_knn(Q, C, D, z_q.data_ptr<float>(), z_cand.data_ptr<float>(), (int32_t)metric, (int32_t)k,
                          f.cand_key, f.src_key, f.excl_ptr, f.excl_key, f.nnz, val.data_ptr<float>(),
                          idx.data_ptr<int64_t>(), return_scores ? all.data_ptr<float>() : nullptr, ws.data_ptr(), nb,
                          cur_stream()),
           "tgnx_embed_knn");
  return {val, idx, all};
}

// LinkPredictor + top-k over a candidate list per source (tgnx_link_predictor_topk_lists):
// (val [B, k], idx [B, k], slot [B, k], logits [nnz] or empty, n_invalid [1])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> predictor_topk_lists(
    const at::Tensor& z_src, const at::Tensor& z_cand, const at::Tensor& w_src, const c10::optional<at::Tensor>& b_src,
    const at::Tensor& w_dst, const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out,
    int64_t k, bool sigmoid, bool return_scores, const at::Tensor& list_ptr, const at::Tensor& list_idx,
    int64_t max_len) {
  const auto [d_in, D] = topk_args(z_src, z_cand, w_src, w_dst, w_out, b_out, k);
  const int64_t B = z_src.size(0), C = z_cand.size(0), nnz = list_idx.numel();
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  dev_tensor(list_ptr, at::kLong, "list_ptr");
  dev_tensor(list_idx, at::kLong, "list_idx");
  TORCH_CHECK(list_ptr.numel() == B + 1, "list_ptr must have n_src + 1 entries");
  TORCH_CHECK(max_len >= 0, "max_len must be >= 0");
  same_device(z_src, {&list_ptr, &list_idx});
  const c10::OptionalDeviceGuard guard(z_src.device());
  at::Tensor val = at::empty({B, k}, z_src.options());
  at::Tensor idx = at::empty({B, k}, z_src.options().dtype(at::kLong));
  at::Tensor slot = at::empty({B, k}, z_src.options().dtype(at::kLong));
  at::Tensor logits = return_scores ? at::empty({nnz}, z_src.options()) : at::empty({0}, z_src.options());
  at::Tensor bad = at::zeros({1}, z_src.options().dtype(at::kLong));
  const size_t nb = tgnx_link_predictor_topk_lists_ws_bytes(B, C, d_in, D, (int32_t)k, max_len);
  at::Tensor ws = at::empty({(int64_t)nb}, z_src.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor_topk_lists(
               B, C, d_in, D, z_src.data_ptr<float>(), z_cand.data_ptr<float>(), w_src.data_ptr<float>(), bs,
               w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(), b_out.data_ptr<float>(), (int32_t)k,
               sigmoid ? 1 : 0, list_ptr.data_ptr<int64_t>(), list_idx.data_ptr<int64_t>(), nnz, max_len,
               val.data_ptr<float>(), idx.data_ptr<int64_t>(), slot.data_ptr<int64_t>(),
               return_scores ? logits.data_ptr<float>() : nullptr, bad.data_ptr<int64_t>(), ws.data_ptr(), nb,
               cur_stream()),
           "tgnx_link_predictor_topk_lists");
  return {val, idx, slot, logits, bad};
}

// where target[q] stands among the first n_count rows of z_cand (tgnx_link_predictor_rank):
// (gt [B], eq [B], n [B] int64, tlogit [B])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> predictor_rank(
    const at::Tensor& z_src, const at::Tensor& z_cand, const at::Tensor& w_src, const c10::optional<at::Tensor>& b_src,
    const at::Tensor& w_dst, const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out,
    const at::Tensor& target, int64_t n_count, const c10::optional<at::Tensor>& cand_key,
    const c10::optional<at::Tensor>& src_key, const c10::optional<at::Tensor>& excl_ptr,
    const c10::optional<at::Tensor>& excl_key) {
  const auto [d_in, D] = topk_args(z_src, z_cand, w_src, w_dst, w_out, b_out, 1);
  const int64_t B = z_src.size(0), C = z_cand.size(0);
  TORCH_CHECK(n_count >= 0 && n_count <= C, "n_count must be in [0, n_cand], got ", n_count);
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  dev_tensor(target, at::kLong, "target");
  TORCH_CHECK(target.numel() == B, "target must have n_src entries");
  same_device(z_src, {&target});
  const KeyArgs f = key_args(z_src, C, cand_key, src_key, excl_ptr, excl_key);
  const c10::OptionalDeviceGuard guard(z_src.device());
  const auto lopt = z_src.options().dtype(at::kLong);
  at::Tensor gt = at::empty({B}, lopt), eq = at::empty({B}, lopt), n = at::empty({B}, lopt);
  at::Tensor tl = at::empty({B}, z_src.options());
  const size_t nb = tgnx_link_predictor_rank_ws_bytes(B, C, d_in, D);
  at::Tensor ws = at::empty({(int64_t)nb}, z_src.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor_rank(B, C, d_in, D, z_src.data_ptr<float>(), z_cand.data_ptr<float>(),
                                    w_src.data_ptr<float>(), bs, w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(),
                                    b_out.data_ptr<float>(), n_count, target.data_ptr<int64_t>(), f.cand_key, f.src_key,
                                    f.excl_ptr, f.excl_key, f.nnz, gt.data_ptr<int64_t>(), eq.data_ptr<int64_t>(),
                                    n.data_ptr<int64_t>(), tl.data_ptr<float>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_link_predictor_rank");
  return {gt, eq, n, tl};
}

// leave-one-out link logits (tgnx_link_predictor_loo, csrc/tgnx_explain.hip):
// (base [P], src_logit [P, K], dst_logit [P, K], status [1] int64: 1 when a row index lay outside [0, n))
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> predictor_loo(
    const at::Tensor& z, const at::Tensor& loo_z, const at::Tensor& count, const at::Tensor& src_row,
    const at::Tensor& dst_row, const at::Tensor& w_src, const c10::optional<at::Tensor>& b_src, const at::Tensor& w_dst,
    const c10::optional<at::Tensor>& b_dst, const at::Tensor& w_out, const at::Tensor& b_out) {
  dev_tensor(z, at::kFloat, "z");
  dev_tensor(loo_z, at::kFloat, "loo_z");
  dev_tensor(count, at::kInt, "count");
  dev_tensor(src_row, at::kLong, "src_row");
  dev_tensor(dst_row, at::kLong, "dst_row");
  dev_tensor(w_src, at::kFloat, "w_src");
  dev_tensor(w_dst, at::kFloat, "w_dst");
  dev_tensor(w_out, at::kFloat, "w_out");
  dev_tensor(b_out, at::kFloat, "b_out");
  TORCH_CHECK(z.dim() == 2 && loo_z.dim() == 3 && loo_z.size(0) == z.size(0) && loo_z.size(2) == z.size(1),
              "z [n, d] and loo_z [n, K, d]");
  const int64_t n = z.size(0), K = loo_z.size(1), d_in = z.size(1), D = w_src.size(0), P = src_row.numel();
  TORCH_CHECK(K >= 1 && K <= 64, "loo_z must have 1 <= K <= 64 rows per node, got ", K);
  TORCH_CHECK(count.numel() == n, "count must have n entries");
  TORCH_CHECK(dst_row.numel() == P, "src_row and dst_row must have the same number of entries");
  TORCH_CHECK(w_src.dim() == 2 && w_src.size(1) == d_in && w_dst.dim() == 2 && w_dst.size(0) == D &&
                  w_dst.size(1) == d_in,
              "w_src / w_dst must be [D, d]");
  TORCH_CHECK(w_out.numel() == D && b_out.numel() == 1, "w_out must have D entries and b_out one");
  same_device(z, {&loo_z, &count, &src_row, &dst_row, &w_src, &w_dst, &w_out, &b_out});
  const float* bs = opt_ptr(b_src, z, D, "b_src");
  const float* bd = opt_ptr(b_dst, z, D, "b_dst");
  const c10::OptionalDeviceGuard guard(z.device());
  at::Tensor base = at::empty({P}, z.options()), sl = at::empty({P, K}, z.options()), dl = at::empty({P, K}, z.options());
  at::Tensor status = at::zeros({1}, z.options().dtype(at::kLong));
  const size_t nb = tgnx_link_predictor_loo_ws_bytes(n, K, P, d_in, D);
  at::Tensor ws = at::empty({(int64_t)nb}, z.options().dtype(at::kByte));
  check_rc(tgnx_link_predictor_loo(n, K, P, d_in, D, z.data_ptr<float>(), loo_z.data_ptr<float>(),
                                   count.data_ptr<int32_t>(), src_row.data_ptr<int64_t>(), dst_row.data_ptr<int64_t>(),
                                   w_src.data_ptr<float>(), bs, w_dst.data_ptr<float>(), bd, w_out.data_ptr<float>(),
                                   b_out.data_ptr<float>(), base.data_ptr<float>(), sl.data_ptr<float>(),
                                   dl.data_ptr<float>(), status.data_ptr<int64_t>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_link_predictor_loo");
  return {base, sl, dl, status};
}

void attn_args(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const c10::optional<at::Tensor>& e,
               const at::Tensor& indptr, int64_t heads) {
  dev_tensor(q, at::kFloat, "q");
  dev_tensor(k, at::kFloat, "k");
  dev_tensor(v, at::kFloat, "v");
  dev_tensor(indptr, at::kLong, "indptr");
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2 && v.sizes() == k.sizes() && k.size(1) == q.size(1),
              "q [n_dst, H*C], k / v [E, H*C]");
  TORCH_CHECK(heads >= 1 && q.size(1) % heads == 0, "H*C must be a multiple of heads");
  TORCH_CHECK(indptr.numel() == q.size(0) + 1, "indptr must have n_dst + 1 entries");
  same_device(q, {&k, &v, &indptr});
  if (e.has_value()) {
    dev_tensor(*e, at::kFloat, "e");
    TORCH_CHECK(e->sizes() == k.sizes(), "e must be [E, H*C]");
    same_device(q, {&*e});
  }
}

// attention dropout's arguments (edge_attn_drop_fwd / _bwd): p, the seed and the optional int64 keys
struct AttnDropArgs {
  float p;
  uint64_t seed, stream;
  const int64_t* dst_key;
  const int64_t* edge_key;
};
const int64_t* key_ptr(const c10::optional<at::Tensor>& x, const at::Tensor& ref, int64_t numel, const char* name) {
  if (!x.has_value()) return nullptr;
  dev_tensor(*x, at::kLong, name);
  TORCH_CHECK(x->dim() == 1 && x->numel() == numel, name, " must be [", numel, "]");
  same_device(ref, {&*x});
  return x->data_ptr<int64_t>();
}
AttnDropArgs attn_drop_args(const at::Tensor& q, const at::Tensor& k, double p, int64_t seed, int64_t stream,
                            const c10::optional<at::Tensor>& dst_key, const c10::optional<at::Tensor>& edge_key) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "p must be finite with 0 <= p < 1, got ", p);
  TORCH_CHECK((float)p < 1.0f, "p rounds to 1 in float32");
  TORCH_CHECK(seed >= 0, "seed must be a non-negative integer below 2^63");
  TORCH_CHECK(stream >= 0, "stream must be non-negative");
  return {(float)p, (uint64_t)seed, (uint64_t)stream, key_ptr(dst_key, q, q.size(0), "dst_key"),
          key_ptr(edge_key, q, k.size(0), "edge_key")};
}

// drop null: tgnx_edge_attn_fwd / _bwd
std::tuple<at::Tensor, at::Tensor> attn_fwd_impl(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                                 const c10::optional<at::Tensor>& e, const at::Tensor& indptr,
                                                 int64_t heads, const AttnDropArgs* drop) {
  const c10::OptionalDeviceGuard guard(q.device());
  const int64_t n = q.size(0), E = k.size(0), C = q.size(1) / heads;
  at::Tensor out = at::empty_like(q), alpha = at::empty({E, heads}, q.options());
  const float* ep = e.has_value() ? e->data_ptr<float>() : nullptr;
  if (drop)
    check_rc(tgnx_edge_attn_drop_fwd(n, E, (int32_t)heads, (int32_t)C, q.data_ptr<float>(), k.data_ptr<float>(),
                                     v.data_ptr<float>(), ep, indptr.data_ptr<int64_t>(), out.data_ptr<float>(),
                                     alpha.data_ptr<float>(), drop->p, drop->seed, drop->stream, drop->dst_key,
                                     drop->edge_key, cur_stream()),
             "tgnx_edge_attn_drop_fwd");
  else
    check_rc(tgnx_edge_attn_fwd(n, E, (int32_t)heads, (int32_t)C, q.data_ptr<float>(), k.data_ptr<float>(),
                                v.data_ptr<float>(), ep, indptr.data_ptr<int64_t>(), out.data_ptr<float>(),
                                alpha.data_ptr<float>(), cur_stream()),
             "tgnx_edge_attn_fwd");
  return {out, alpha};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> attn_bwd_impl(
    const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const c10::optional<at::Tensor>& e, const at::Tensor& indptr, const at::Tensor& alpha, int64_t heads,
    const AttnDropArgs* drop) {
  const c10::OptionalDeviceGuard guard(q.device());
  const int64_t n = q.size(0), E = k.size(0), C = q.size(1) / heads;
  at::Tensor dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  at::Tensor de = e.has_value() ? at::empty_like(k) : at::empty({0}, k.options());
  const float* ep = e.has_value() ? e->data_ptr<float>() : nullptr;
  float* dep = e.has_value() ? de.data_ptr<float>() : nullptr;
  if (drop)
    check_rc(tgnx_edge_attn_drop_bwd(n, E, (int32_t)heads, (int32_t)C, dout.data_ptr<float>(), q.data_ptr<float>(),
                                     k.data_ptr<float>(), v.data_ptr<float>(), ep, indptr.data_ptr<int64_t>(),
                                     alpha.data_ptr<float>(), dq.data_ptr<float>(), dk.data_ptr<float>(),
                                     dv.data_ptr<float>(), dep, drop->p, drop->seed, drop->stream, drop->dst_key,
                                     drop->edge_key, cur_stream()),
             "tgnx_edge_attn_drop_bwd");
  else
    check_rc(tgnx_edge_attn_bwd(n, E, (int32_t)heads, (int32_t)C, dout.data_ptr<float>(), q.data_ptr<float>(),
                                k.data_ptr<float>(), v.data_ptr<float>(), ep, indptr.data_ptr<int64_t>(),
                                alpha.data_ptr<float>(), dq.data_ptr<float>(), dk.data_ptr<float>(),
                                dv.data_ptr<float>(), dep, cur_stream()),
             "tgnx_edge_attn_bwd");
  return {dq, dk, dv, de};
}

void attn_bwd_args(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& alpha,
                   int64_t heads) {
  dev_tensor(dout, at::kFloat, "dout");
  dev_tensor(alpha, at::kFloat, "alpha");
  TORCH_CHECK(dout.sizes() == q.sizes(), "dout must be [n_dst, H*C]");
  TORCH_CHECK(alpha.dim() == 2 && alpha.size(0) == k.size(0) && alpha.size(1) == heads, "alpha must be [E, heads]");
  same_device(q, {&dout, &alpha});
}

std::tuple<at::Tensor, at::Tensor> edge_attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                                 const c10::optional<at::Tensor>& e, const at::Tensor& indptr,
                                                 int64_t heads) {
  attn_args(q, k, v, e, indptr, heads);
  return attn_fwd_impl(q, k, v, e, indptr, heads, nullptr);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> edge_attn_bwd(
    const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const c10::optional<at::Tensor>& e, const at::Tensor& indptr, const at::Tensor& alpha, int64_t heads) {
  attn_args(q, k, v, e, indptr, heads);
  attn_bwd_args(dout, q, k, alpha, heads);
  return attn_bwd_impl(dout, q, k, v, e, indptr, alpha, heads, nullptr);
}

std::tuple<at::Tensor, at::Tensor> edge_attn_drop_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                                      const c10::optional<at::Tensor>& e, const at::Tensor& indptr,
                                                      int64_t heads, double p, int64_t seed, int64_t stream,
                                                      const c10::optional<at::Tensor>& dst_key,
                                                      const c10::optional<at::Tensor>& edge_key) {
  attn_args(q, k, v, e, indptr, heads);
  const AttnDropArgs d = attn_drop_args(q, k, p, seed, stream, dst_key, edge_key);
  return attn_fwd_impl(q, k, v, e, indptr, heads, &d);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> edge_attn_drop_bwd(
    const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const c10::optional<at::Tensor>& e, const at::Tensor& indptr, const at::Tensor& alpha, int64_t heads, double p,
    int64_t seed, int64_t stream, const c10::optional<at::Tensor>& dst_key,
    const c10::optional<at::Tensor>& edge_key) {
  attn_args(q, k, v, e, indptr, heads);
  attn_bwd_args(dout, q, k, alpha, heads);
  const AttnDropArgs d = attn_drop_args(q, k, p, seed, stream, dst_key, edge_key);
  return attn_bwd_impl(dout, q, k, v, e, indptr, alpha, heads, &d);
}

// ------------------------------------------------------------------ backward ops (csrc/tgnx_ops_bwd.hip)
// A gradient the caller does not need (need[i] == 0) is not computed and comes back as an empty tensor.
at::Tensor ws_bytes(const at::Tensor& ref, size_t nb) {
  return at::empty({(int64_t)std::max<size_t>(nb, 1)}, ref.options().dtype(at::kByte));
}
at::Tensor grad_like(bool need, at::IntArrayRef shape, const at::Tensor& ref) {
  return need ? at::empty(shape, ref.options()) : at::empty({0}, ref.options());
}
float* grad_ptr(bool need, at::Tensor& g) { return need ? g.data_ptr<float>() : nullptr; }

// x [M, N] with unit column stride; rows may be strided (a column slice of a wider matrix)
at::Tensor col_sum(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "x must be a HIP device tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat, "x has dtype ", x.scalar_type(), ", expected ", at::kFloat);
  TORCH_CHECK(x.dim() == 2, "x must be 2-D");
  const int64_t M = x.size(0), N = x.size(1);
  const int64_t ldx = M > 1 ? x.stride(0) : N;
  TORCH_CHECK(N <= 1 || x.stride(1) == 1, "x must have unit column stride");
  TORCH_CHECK(ldx >= N, "x's rows must not overlap (row stride ", ldx, " < ", N, " columns)");
  const c10::OptionalDeviceGuard guard(x.device());
  at::Tensor out = at::empty({N}, x.options());
  const size_t nb = tgnx_col_sum_ws_bytes(M, N);
  at::Tensor ws = ws_bytes(x, nb);
  check_rc(tgnx_col_sum(M, N, x.data_ptr<float>(), ldx, out.data_ptr<float>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_col_sum");
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> gru_update_bwd(
    const at::Tensor& dh_out, const at::Tensor& x, const at::Tensor& h, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const c10::optional<at::Tensor>& b_ih, const c10::optional<at::Tensor>& b_hh,
    int64_t cell, at::IntArrayRef need) {
  dev_tensor(dh_out, at::kFloat, "dh_out");
  dev_tensor(x, at::kFloat, "x");
  dev_tensor(h, at::kFloat, "h");
  dev_tensor(w_ih, at::kFloat, "w_ih");
  dev_tensor(w_hh, at::kFloat, "w_hh");
  TORCH_CHECK(cell == 0 || cell == 1, "cell 0 (GRUCell) or 1 (RNNCell, tanh)");
  TORCH_CHECK(need.size() == 6, "need must have 6 entries (dx, dh, dw_ih, dw_hh, db_ih, db_hh)");
  TORCH_CHECK(x.dim() == 2 && h.dim() == 2 && x.size(0) == h.size(0), "x [M, d_in] and h [M, D]");
  TORCH_CHECK(dh_out.sizes() == h.sizes(), "dh_out must be [M, D]");
  const int64_t M = x.size(0), d_in = x.size(1), D = h.size(1), G = (cell == 0 ? 3 : 1) * D;
  TORCH_CHECK(w_ih.dim() == 2 && w_ih.size(0) == G && w_ih.size(1) == d_in, "w_ih must be [", G, ", ", d_in, "]");
  TORCH_CHECK(w_hh.dim() == 2 && w_hh.size(0) == G && w_hh.size(1) == D, "w_hh must be [", G, ", ", D, "]");
  same_device(x, {&dh_out, &h, &w_ih, &w_hh});
  const float* bi = opt_ptr(b_ih, x, G, "b_ih");
  const float* bh = opt_ptr(b_hh, x, G, "b_hh");
  const c10::OptionalDeviceGuard guard(x.device());
  at::Tensor dx = grad_like(need[0], x.sizes(), x), dh = grad_like(need[1], h.sizes(), x);
  at::Tensor dwi = grad_like(need[2], w_ih.sizes(), x), dwh = grad_like(need[3], w_hh.sizes(), x);
  at::Tensor dbi = grad_like(need[4], {G}, x), dbh = grad_like(need[5], {G}, x);
  const size_t nb = tgnx_memory_cell_bwd_ws_bytes(M, d_in, D);
  at::Tensor ws = ws_bytes(x, nb);
  check_rc(tgnx_memory_cell_bwd((int32_t)cell, M, d_in, D, dh_out.data_ptr<float>(), x.data_ptr<float>(),
                                h.data_ptr<float>(), w_ih.data_ptr<float>(), w_hh.data_ptr<float>(), bi, bh,
                                grad_ptr(need[0], dx), grad_ptr(need[1], dh), grad_ptr(need[2], dwi),
                                grad_ptr(need[3], dwh), grad_ptr(need[4], dbi), grad_ptr(need[5], dbh), ws.data_ptr(),
                                nb, cur_stream()),
           "tgnx_memory_cell_bwd");
  return {dx, dh, dwi, dwh, dbi, dbh};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
predictor_bwd(const at::Tensor& dout, const at::Tensor& z_src, const at::Tensor& z_dst, const at::Tensor& w_src,
              const c10::optional<at::Tensor>& b_src, const at::Tensor& w_dst, const c10::optional<at::Tensor>& b_dst,
              const at::Tensor& w_out, const at::Tensor& b_out, bool sigmoid, at::IntArrayRef need) {
  dev_tensor(dout, at::kFloat, "dout");
  dev_tensor(z_src, at::kFloat, "z_src");
  dev_tensor(z_dst, at::kFloat, "z_dst");
  dev_tensor(w_src, at::kFloat, "w_src");
  dev_tensor(w_dst, at::kFloat, "w_dst");
  dev_tensor(w_out, at::kFloat, "w_out");
  dev_tensor(b_out, at::kFloat, "b_out");
  TORCH_CHECK(need.size() == 8,
              "need must have 8 entries (dz_src, dz_dst, dw_src, db_src, dw_dst, db_dst, dw_out, db_out)");
  TORCH_CHECK(z_src.dim() == 2 && z_dst.dim() == 2 && z_src.size(1) == z_dst.size(1), "z_src [B, d] and z_dst [M, d]");
  TORCH_CHECK(w_src.dim() == 2 && w_dst.dim() == 2, "w_src / w_dst must be [D, d]");
  const int64_t B = z_src.size(0), M = z_dst.size(0), d_in = z_src.size(1), D = w_src.size(0);
  TORCH_CHECK(M == 0 || (B > 0 && M % B == 0), "z_dst rows must be a multiple of z_src rows (tile pairing)");
  TORCH_CHECK(w_src.size(1) == d_in && w_dst.size(0) == D && w_dst.size(1) == d_in, "w_src / w_dst must be [D, d]");
  TORCH_CHECK(w_out.numel() == D && b_out.numel() == 1, "w_out must have D entries and b_out one");
  TORCH_CHECK(dout.numel() == M, "dout must have one entry per z_dst row");
  same_device(z_src, {&dout, &z_dst, &w_src, &w_dst, &w_out, &b_out});
  const float* bs = opt_ptr(b_src, z_src, D, "b_src");
  const float* bd = opt_ptr(b_dst, z_src, D, "b_dst");
  const c10::OptionalDeviceGuard guard(z_src.device());
  at::Tensor dzs = grad_like(need[0], z_src.sizes(), z_src), dzd = grad_like(need[1], z_dst.sizes(), z_src);
  at::Tensor dws = grad_like(need[2], w_src.sizes(), z_src), dbs = grad_like(need[3], {D}, z_src);
  at::Tensor dwd = grad_like(need[4], w_dst.sizes(), z_src), dbd = grad_like(need[5], {D}, z_src);
  at::Tensor dwo = grad_like(need[6], w_out.sizes(), z_src), dbo = grad_like(need[7], b_out.sizes(), z_src);
  const size_t nb = tgnx_link_predictor_bwd_ws_bytes(B, M, d_in, D);
  at::Tensor ws = ws_bytes(z_src, nb);
  check_rc(tgnx_link_predictor_bwd(B, M, d_in, D, dout.data_ptr<float>(), z_src.data_ptr<float>(),
                                   z_dst.data_ptr<float>(), w_src.data_ptr<float>(), bs, w_dst.data_ptr<float>(), bd,
                                   w_out.data_ptr<float>(), b_out.data_ptr<float>(), sigmoid ? 1 : 0,
                                   grad_ptr(need[0], dzs), grad_ptr(need[1], dzd), grad_ptr(need[2], dws),
                                   grad_ptr(need[3], dbs), grad_ptr(need[4], dwd), grad_ptr(need[5], dbd),
                                   grad_ptr(need[6], dwo), grad_ptr(need[7], dbo), ws.data_ptr(), nb, cur_stream()),
           "tgnx_link_predictor_bwd");
  return {dzs, dzd, dws, dbs, dwd, dbd, dwo, dbo};
}

// NodePredictor (decoder.py:30-41; csrc/tgnx_nodeprop.hip): (logits [M, C], h [M, D] or an empty tensor)
void node_head_args(const at::Tensor& z, const at::Tensor& w1, const at::Tensor& w2) {
  dev_tensor(z, at::kFloat, "z");
  dev_tensor(w1, at::kFloat, "w1");
  dev_tensor(w2, at::kFloat, "w2");
  TORCH_CHECK(z.dim() == 2 && w1.dim() == 2 && w2.dim() == 2, "z [M, D], w1 [D, D], w2 [C, D]");
  const int64_t D = z.size(1);
  TORCH_CHECK(w1.size(0) == D && w1.size(1) == D && w2.size(1) == D, "z [M, D], w1 [D, D], w2 [C, D]");
  same_device(z, {&w1, &w2});
}

std::tuple<at::Tensor, at::Tensor> node_predictor(const at::Tensor& z, const at::Tensor& w1,
                                                  const c10::optional<at::Tensor>& b1, const at::Tensor& w2,
                                                  const c10::optional<at::Tensor>& b2, bool need_h) {
  node_head_args(z, w1, w2);
  const int64_t M = z.size(0), D = z.size(1), C = w2.size(0);
  const float* p1 = opt_ptr(b1, z, D, "b1");
  const float* p2 = opt_ptr(b2, z, C, "b2");
  const c10::OptionalDeviceGuard guard(z.device());
  at::Tensor logits = at::empty({M, C}, z.options()), h = grad_like(need_h, {M, D}, z);
  const size_t nb = tgnx_node_predictor_ws_bytes(M, D, C);
  at::Tensor ws = ws_bytes(z, nb);
  check_rc(tgnx_node_predictor(M, D, C, z.data_ptr<float>(), w1.data_ptr<float>(), p1, w2.data_ptr<float>(), p2,
                               logits.data_ptr<float>(), grad_ptr(need_h, h), ws.data_ptr(), nb, cur_stream()),
           "tgnx_node_predictor");
  return {logits, h};
}

// (dz, dw1, db1, dw2, db2); an empty tensor for a gradient that need[i] = 0 leaves out
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> node_predictor_bwd(
    const at::Tensor& dlogits, const at::Tensor& z, const at::Tensor& h, const at::Tensor& w1, const at::Tensor& w2,
    at::IntArrayRef need) {
  node_head_args(z, w1, w2);
  dev_tensor(dlogits, at::kFloat, "dlogits");
  dev_tensor(h, at::kFloat, "h");
  TORCH_CHECK(need.size() == 5, "need must have 5 entries (dz, dw1, db1, dw2, db2)");
  const int64_t M = z.size(0), D = z.size(1), C = w2.size(0);
  TORCH_CHECK(dlogits.dim() == 2 && dlogits.size(0) == M && dlogits.size(1) == C, "dlogits must be [M, C]");
  TORCH_CHECK(h.dim() == 2 && h.size(0) == M && h.size(1) == D, "h must be [M, D] (the forward's hidden rows)");
  same_device(z, {&dlogits, &h});
  const c10::OptionalDeviceGuard guard(z.device());
  at::Tensor dz = grad_like(need[0], z.sizes(), z), dw1 = grad_like(need[1], w1.sizes(), z);
  at::Tensor db1 = grad_like(need[2], {D}, z), dw2 = grad_like(need[3], w2.sizes(), z), db2 = grad_like(need[4], {C}, z);
  const size_t nb = tgnx_node_predictor_bwd_ws_bytes(M, D, C);
  at::Tensor ws = ws_bytes(z, nb);
  check_rc(tgnx_node_predictor_bwd(M, D, C, dlogits.data_ptr<float>(), z.data_ptr<float>(), h.data_ptr<float>(),
                                   w1.data_ptr<float>(), w2.data_ptr<float>(), grad_ptr(need[0], dz),
                                   grad_ptr(need[1], dw1), grad_ptr(need[2], db1), grad_ptr(need[3], dw2),
                                   grad_ptr(need[4], db2), ws.data_ptr(), nb, cur_stream()),
           "tgnx_node_predictor_bwd");
  return {dz, dw1, db1, dw2, db2};
}

// the row kernel (tgnx_node_loss_ndcg): (mean loss [], loss rows [M], dlogits [M, C], ndcg float64 [M]); a part that
// is not asked for comes back as an empty tensor.  cum: k + 1 float64 on the device (tgnx/ops.py builds it).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> node_loss_ndcg(const at::Tensor& logits, const at::Tensor& y,
                                                                          const at::Tensor& cum, int64_t k,
                                                                          bool need_loss, bool need_grad,
                                                                          bool need_ndcg) {
  dev_tensor(logits, at::kFloat, "logits");
  dev_tensor(y, at::kFloat, "y");
  dev_tensor(cum, at::kDouble, "cum");
  TORCH_CHECK(logits.dim() == 2 && y.sizes() == logits.sizes(), "logits and y must be [M, C]");
  TORCH_CHECK(k >= 1 && k <= TGNX_NODE_MAX_K, "k must be in [1, ", TGNX_NODE_MAX_K, "], got ", k);
  TORCH_CHECK(cum.numel() == k + 1, "cum must have k + 1 entries");
  same_device(logits, {&y, &cum});
  const int64_t M = logits.size(0), C = logits.size(1);
  const c10::OptionalDeviceGuard guard(logits.device());
  at::Tensor mean = grad_like(need_loss, {}, logits), rows = grad_like(need_loss, {M}, logits);
  at::Tensor dl = grad_like(need_grad, logits.sizes(), logits);
  at::Tensor nd = need_ndcg ? at::empty({M}, cum.options()) : at::empty({0}, cum.options());
  check_rc(tgnx_node_loss_ndcg(M, C, (int32_t)k, logits.data_ptr<float>(), y.data_ptr<float>(),
                               cum.data_ptr<double>(), M > 0 ? 1.0f / (float)M : 0.0f, grad_ptr(need_loss, rows),
                               grad_ptr(need_loss, mean), grad_ptr(need_grad, dl),
                               need_ndcg ? nd.data_ptr<double>() : nullptr, cur_stream()),
           "tgnx_node_loss_ndcg");
  return {mean, rows, dl, nd};
}

// t [n]; w ([D] or Linear(1, D)'s [D, 1]) and b [D]
int64_t time_args(const at::Tensor& t, const at::Tensor& w, const at::Tensor& b) {
  dev_tensor(t, at::kFloat, "t");
  dev_tensor(w, at::kFloat, "w");
  dev_tensor(b, at::kFloat, "b");
  TORCH_CHECK(t.dim() == 1, "t must be [n]");
  TORCH_CHECK(b.dim() == 1 && w.numel() == b.numel(), "w and b must have D entries each");
  same_device(t, {&w, &b});
  return b.numel();
}

at::Tensor time_encode(const at::Tensor& t, const at::Tensor& w, const at::Tensor& b) {
  const int64_t D = time_args(t, w, b), n = t.numel();
  const c10::OptionalDeviceGuard guard(t.device());
  at::Tensor out = at::empty({n, D}, t.options());
  check_rc(tgnx_time_encode(n, D, t.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
                            out.data_ptr<float>(), cur_stream()),
           "tgnx_time_encode");
  return out;
}

std::tuple<at::Tensor, at::Tensor> time_encode_bwd(const at::Tensor& dout, const at::Tensor& t, const at::Tensor& w,
                                                   const at::Tensor& b) {
  const int64_t D = time_args(t, w, b), n = t.numel();
  dev_tensor(dout, at::kFloat, "dout");
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == n && dout.size(1) == D, "dout must be [n, D]");
  same_device(t, {&dout});
  const c10::OptionalDeviceGuard guard(t.device());
  at::Tensor dw = at::empty_like(w), db = at::empty_like(b);
  const size_t nb = tgnx_time_encode_bwd_ws_bytes(n, D);
  at::Tensor ws = ws_bytes(t, nb);
  check_rc(tgnx_time_encode_bwd(n, D, t.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
                                dout.data_ptr<float>(), dw.data_ptr<float>(), db.data_ptr<float>(), ws.data_ptr(), nb,
                                cur_stream()),
           "tgnx_time_encode_bwd");
  return {dw, db};
}

at::Tensor time_embedding(const at::Tensor& x, const at::Tensor& rel_t, const at::Tensor& w, const at::Tensor& b) {
  const int64_t D = time_args(rel_t, w, b), n = rel_t.numel();
  dev_tensor(x, at::kFloat, "x");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == n && x.size(1) == D, "x must be [n, D]");
  same_device(rel_t, {&x});
  const c10::OptionalDeviceGuard guard(x.device());
  at::Tensor out = at::empty_like(x);
  check_rc(tgnx_time_embedding(n, D, x.data_ptr<float>(), rel_t.data_ptr<float>(), w.data_ptr<float>(),
                               b.data_ptr<float>(), out.data_ptr<float>(), cur_stream()),
           "tgnx_time_embedding");
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> time_embedding_bwd(const at::Tensor& dout, const at::Tensor& x,
                                                                  const at::Tensor& rel_t, const at::Tensor& w,
                                                                  const at::Tensor& b, bool need_dx) {
  const int64_t D = time_args(rel_t, w, b), n = rel_t.numel();
  dev_tensor(x, at::kFloat, "x");
  dev_tensor(dout, at::kFloat, "dout");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == n && x.size(1) == D, "x must be [n, D]");
  TORCH_CHECK(dout.sizes() == x.sizes(), "dout must be [n, D]");
  same_device(rel_t, {&x, &dout});
  const c10::OptionalDeviceGuard guard(x.device());
  at::Tensor dx = grad_like(need_dx, x.sizes(), x), dw = at::empty_like(w), db = at::empty_like(b);
  const size_t nb = tgnx_time_embedding_bwd_ws_bytes(n, D);
  at::Tensor ws = ws_bytes(x, nb);
  check_rc(tgnx_time_embedding_bwd(n, D, x.data_ptr<float>(), rel_t.data_ptr<float>(), w.data_ptr<float>(),
                                   b.data_ptr<float>(), dout.data_ptr<float>(), grad_ptr(need_dx, dx),
                                   dw.data_ptr<float>(), db.data_ptr<float>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_time_embedding_bwd");
  return {dx, dw, db};
}

at::Tensor msg_agg_last_bwd(const at::Tensor& dout, const at::Tensor& argmax, int64_t n_msg) {
  dev_tensor(dout, at::kFloat, "dout");
  dev_tensor(argmax, at::kLong, "argmax");
  TORCH_CHECK(dout.dim() == 2, "dout must be [dim_size, dim]");
  TORCH_CHECK(argmax.dim() == 1 && argmax.numel() == dout.size(0), "argmax must be [dim_size]");
  TORCH_CHECK(n_msg >= 0, "n_msg must be non-negative");
  same_device(dout, {&argmax});
  const c10::OptionalDeviceGuard guard(dout.device());
  at::Tensor dmsg = at::empty({n_msg, dout.size(1)}, dout.options());
  check_rc(tgnx_msg_agg_last_bwd(dout.data_ptr<float>(), argmax.data_ptr<int64_t>(), dout.size(0), dout.size(1), n_msg,
                                 dmsg.data_ptr<float>(), cur_stream()),
           "tgnx_msg_agg_last_bwd");
  return dmsg;
}

// out-of-range index -> RuntimeError, as the forward (one device -> host read of the drop count)
at::Tensor msg_agg_mean_bwd(const at::Tensor& dout, const at::Tensor& index) {
  dev_tensor(dout, at::kFloat, "dout");
  dev_tensor(index, at::kLong, "index");
  TORCH_CHECK(dout.dim() == 2, "dout must be [dim_size, dim]");
  TORCH_CHECK(index.dim() == 1, "index must be [n_msg]");
  same_device(dout, {&index});
  const c10::OptionalDeviceGuard guard(dout.device());
  const int64_t n = index.numel(), dim_size = dout.size(0), dim = dout.size(1);
  at::Tensor dmsg = at::empty({n, dim}, dout.options());
  at::Tensor bad = at::zeros({1}, index.options());
  const size_t nb = tgnx_msg_agg_mean_bwd_ws_bytes(dim_size);
  at::Tensor ws = ws_bytes(dout, nb);
  check_rc(tgnx_msg_agg_mean_bwd(dout.data_ptr<float>(), index.data_ptr<int64_t>(), n, dim, dim_size,
                                 dmsg.data_ptr<float>(), bad.data_ptr<int64_t>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_msg_agg_mean_bwd");
  const int64_t nbad = bad.cpu().data_ptr<int64_t>()[0];
  TORCH_CHECK(nbad == 0, "msg_agg_mean_bwd: ", nbad, " index entries outside [0, ", dim_size, ")");
  return dmsg;
}

// ------------------------------------------------------------------ device message store (csrc/tgnx_memstore.hip)
// The store's tensors (tgnx.nn.TGNMemory's non-persistent buffers): log_src / log_dst / log_t int64[cap], log_raw
// fp32[cap, d], arena int64[2 cap], node_tab int64[4 N], bad int64[1].
void store_log(const at::Tensor& log_src, const at::Tensor& log_dst, const at::Tensor& log_t,
               const at::Tensor& log_raw) {
  dev_tensor(log_src, at::kLong, "log_src");
  dev_tensor(log_dst, at::kLong, "log_dst");
  dev_tensor(log_t, at::kLong, "log_t");
  dev_tensor(log_raw, at::kFloat, "log_raw");
  TORCH_CHECK(log_src.dim() == 1 && log_dst.sizes() == log_src.sizes() && log_t.sizes() == log_src.sizes() &&
                  log_raw.dim() == 2 && log_raw.size(0) == log_src.size(0),
              "the event log must be src, dst, t [cap] and raw_msg [cap, d]");
  same_device(log_src, {&log_dst, &log_t, &log_raw});
}

void memstore_put(const at::Tensor& src, const at::Tensor& dst, const at::Tensor& t, const at::Tensor& raw_msg,
                  const at::Tensor& sorted, const at::Tensor& perm, int64_t start, at::Tensor log_src,
                  at::Tensor log_dst, at::Tensor log_t, at::Tensor log_raw, at::Tensor arena, at::Tensor node_tab,
                  at::Tensor bad) {
  store_log(log_src, log_dst, log_t, log_raw);
  dev_tensor(src, at::kLong, "src");
  dev_tensor(dst, at::kLong, "dst");
  dev_tensor(t, at::kLong, "t");
  dev_tensor(raw_msg, at::kFloat, "raw_msg");
  dev_tensor(sorted, at::kLong, "sorted");
  dev_tensor(perm, at::kLong, "perm");
  dev_tensor(arena, at::kLong, "arena");
  dev_tensor(node_tab, at::kLong, "node_tab");
  dev_tensor(bad, at::kLong, "bad");
  same_device(log_src, {&src, &dst, &t, &raw_msg, &sorted, &perm, &arena, &node_tab, &bad});
  const int64_t B = src.numel(), cap = log_src.size(0), d = log_raw.size(1);
  TORCH_CHECK(dst.numel() == B && t.numel() == B, "src, dst, t must have the same length");
  TORCH_CHECK(raw_msg.dim() == 2 && raw_msg.size(0) == B && raw_msg.size(1) == d, "raw_msg must be [B, ", d, "]");
  TORCH_CHECK(sorted.numel() == 2 * B && perm.numel() == 2 * B, "sorted and perm must be [2, B]");
  TORCH_CHECK(arena.numel() == 2 * cap, "arena must have 2 cap entries");
  TORCH_CHECK(node_tab.numel() % 4 == 0 && bad.numel() >= 1, "node_tab must be [4 N] and bad [1]");
  const c10::OptionalDeviceGuard guard(log_src.device());
  check_rc(tgnx_memstore_put(src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), t.data_ptr<int64_t>(),
                             raw_msg.data_ptr<float>(), B, d, sorted.data_ptr<int64_t>(), perm.data_ptr<int64_t>(),
                             start, cap, node_tab.numel() / 4, log_src.data_ptr<int64_t>(),
                             log_dst.data_ptr<int64_t>(), log_t.data_ptr<int64_t>(), log_raw.data_ptr<float>(),
                             arena.data_ptr<int64_t>(), node_tab.data_ptr<int64_t>(), bad.data_ptr<int64_t>(),
                             cur_stream()),
           "tgnx_memstore_put");
}

// (totals int64[3] = {n_s, n_d, invalid ids} on the device, the workspace memstore_gather continues from): no
// device -> host read here; the caller reads totals once to size the gather
std::tuple<at::Tensor, at::Tensor> memstore_count(const at::Tensor& node_tab, const at::Tensor& n_id,
                                                  const c10::optional<at::Tensor>& put_bad) {
  dev_tensor(node_tab, at::kLong, "node_tab");
  dev_tensor(n_id, at::kLong, "n_id");
  TORCH_CHECK(node_tab.numel() % 4 == 0 && n_id.dim() == 1, "node_tab must be [4 N] and n_id [M]");
  same_device(node_tab, {&n_id});
  const int64_t* pb = nullptr;
  if (put_bad.has_value()) {
    dev_tensor(*put_bad, at::kLong, "put_bad");
    TORCH_CHECK(put_bad->numel() >= 1, "put_bad must be [1]");
    same_device(node_tab, {&*put_bad});
    pb = put_bad->data_ptr<int64_t>();
  }
  const c10::OptionalDeviceGuard guard(node_tab.device());
  const int64_t M = n_id.numel();
  at::Tensor totals = at::empty({3}, n_id.options());
  const size_t nb = tgnx_memstore_gather_ws_bytes(M);
  at::Tensor ws = ws_bytes(node_tab, nb);
  check_rc(tgnx_memstore_count(node_tab.data_ptr<int64_t>(), node_tab.numel() / 4, n_id.data_ptr<int64_t>(), M, pb,
                               totals.data_ptr<int64_t>(), ws.data_ptr(), nb, cur_stream()),
           "tgnx_memstore_count");
  return {totals, ws};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> memstore_gather(const at::Tensor& node_tab,
                                                                           const at::Tensor& arena,
                                                                           const at::Tensor& log_t, int64_t fill,
                                                                           const at::Tensor& n_id, int64_t n_s,
                                                                           int64_t n_d, const at::Tensor& ws) {
  dev_tensor(node_tab, at::kLong, "node_tab");
  dev_tensor(arena, at::kLong, "arena");
  dev_tensor(log_t, at::kLong, "log_t");
  dev_tensor(n_id, at::kLong, "n_id");
  dev_tensor(ws, at::kByte, "ws");
  TORCH_CHECK(node_tab.numel() % 4 == 0 && n_id.dim() == 1, "node_tab must be [4 N] and n_id [M]");
  TORCH_CHECK(fill >= 0 && fill <= log_t.numel() && arena.numel() >= 2 * fill, "fill beyond the log's capacity");
  TORCH_CHECK(n_s >= 0 && n_d >= 0, "n_s and n_d must be non-negative");
  same_device(node_tab, {&arena, &log_t, &n_id, &ws});
  const c10::OptionalDeviceGuard guard(node_tab.device());
  const int64_t M = n_id.numel(), n = n_s + n_d;
  auto lopt = n_id.options();
  at::Tensor slot = at::empty({n}, lopt), owner = at::empty({n}, lopt), t = at::empty({n}, lopt);
  at::Tensor lu = at::empty({M}, lopt);
  check_rc(tgnx_memstore_gather(node_tab.data_ptr<int64_t>(), node_tab.numel() / 4, arena.data_ptr<int64_t>(),
                                log_t.data_ptr<int64_t>(), fill, n_id.data_ptr<int64_t>(), M, n_s, n_d,
                                slot.data_ptr<int64_t>(), owner.data_ptr<int64_t>(), t.data_ptr<int64_t>(),
                                lu.data_ptr<int64_t>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
           "tgnx_memstore_gather");
  return {slot, owner, t, lu};
}

// (rows [n_msg, 2 D + d + T], t_rel [n_msg]); emb / assoc / stamp / n_id: DyRepMemory's embeddings in messages
std::tuple<at::Tensor, at::Tensor> memstore_build_msg(
    const at::Tensor& slot, int64_t n_s, const at::Tensor& log_src, const at::Tensor& log_dst, const at::Tensor& log_t,
    const at::Tensor& log_raw, int64_t fill, const at::Tensor& memory, const at::Tensor& last_update,
    const at::Tensor& w, const at::Tensor& b, const c10::optional<at::Tensor>& emb,
    const c10::optional<at::Tensor>& assoc, const c10::optional<at::Tensor>& stamp,
    const c10::optional<at::Tensor>& n_id, int64_t emb_flags) {
  store_log(log_src, log_dst, log_t, log_raw);
  dev_tensor(slot, at::kLong, "slot");
  dev_tensor(memory, at::kFloat, "memory");
  dev_tensor(last_update, at::kLong, "last_update");
  dev_tensor(w, at::kFloat, "w");
  dev_tensor(b, at::kFloat, "b");
  TORCH_CHECK(memory.dim() == 2 && last_update.dim() == 1 && last_update.numel() == memory.size(0),
              "memory must be [N, D] and last_update [N]");
  TORCH_CHECK(b.dim() == 1 && w.numel() == b.numel(), "w and b must have T entries each");
  TORCH_CHECK(slot.dim() == 1 && n_s >= 0 && n_s <= slot.numel(), "slot must be [n_msg] and 0 <= n_s <= n_msg");
  TORCH_CHECK(fill >= 0 && fill <= log_src.numel(), "fill beyond the log's capacity");
  same_device(slot, {&log_src, &memory, &last_update, &w, &b});
  const int64_t N = memory.size(0), D = memory.size(1), d = log_raw.size(1), T = b.numel(), n = slot.numel();
  const float* pe = nullptr;
  const int64_t *pa = nullptr, *ps = nullptr, *pn = nullptr;
  int64_t E = 0, M = 0;
  if (emb.has_value() && emb_flags != 0) {
    TORCH_CHECK(assoc.has_value() && stamp.has_value() && n_id.has_value(),
                "embeddings in messages need assoc, the stamps and n_id");
    dev_tensor(*emb, at::kFloat, "embeddings");
    dev_tensor(*assoc, at::kLong, "assoc");
    dev_tensor(*stamp, at::kLong, "stamp");
    dev_tensor(*n_id, at::kLong, "n_id");
    TORCH_CHECK(emb->dim() == 2 && emb->size(1) == D, "embeddings must be [*, ", D, "] (the memory's width)");
    TORCH_CHECK(assoc->numel() >= N && stamp->numel() >= N, "assoc and the stamps must have num_nodes entries");
    same_device(slot, {&*emb, &*assoc, &*stamp, &*n_id});
    pe = emb->data_ptr<float>(), pa = assoc->data_ptr<int64_t>(), ps = stamp->data_ptr<int64_t>();
    pn = n_id->data_ptr<int64_t>(), E = emb->size(0), M = n_id->numel();
  }
  const c10::OptionalDeviceGuard guard(slot.device());
  at::Tensor out = at::empty({n, 2 * D + d + T}, memory.options()), t_rel = at::empty({n}, memory.options());
  check_rc(tgnx_memstore_build_msg(slot.data_ptr<int64_t>(), n, n_s, log_src.data_ptr<int64_t>(),
                                   log_dst.data_ptr<int64_t>(), log_t.data_ptr<int64_t>(), log_raw.data_ptr<float>(),
                                   fill, N, D, d, T, memory.data_ptr<float>(), last_update.data_ptr<int64_t>(),
                                   w.data_ptr<float>(), b.data_ptr<float>(), pe, E, pa, ps, pn, M,
                                   (int32_t)(pe ? emb_flags : 0), out.data_ptr<float>(), t_rel.data_ptr<float>(),
                                   cur_stream()),
           "tgnx_memstore_build_msg");
  return {out, t_rel};
}

}  // namespace

TORCH_LIBRARY(tgnx, m) {
  m.def("ring_reset(Tensor(a!) e_id, Tensor(b!) t) -> ()", &ring_reset);
  m.def("ring_sample(Tensor nbr, Tensor e_id, Tensor t, Tensor(a!) assoc, Tensor n_id) -> (Tensor, Tensor, Tensor, Tensor)",
        &ring_sample);
  m.def("ring_insert(Tensor(a!) nbr, Tensor(b!) e_id, Tensor(c!) t, Tensor src, Tensor dst, Tensor ev_t, int cur_e_id, "
        "Tensor(d!) assoc) -> ()",
        &ring_insert);
  m.def("neg_sample(Tensor dst_nodes, Tensor pos, int seed, int offset) -> Tensor", &neg_sample);
  m.def("block_ids(Tensor src, Tensor dst, int batch) -> Tensor", &block_ids);
  m.def("tcsr_build(Tensor src, Tensor dst, Tensor t, int num_nodes, bool add_reverse) -> "
        "(Tensor, Tensor, Tensor, Tensor, bool)",
        &tcsr_build);
  m.def("tcsr_sample(Tensor indptr, Tensor indices, Tensor eid, Tensor ts, int K, Tensor roots, int mode, Tensor cut) "
        "-> (Tensor, Tensor, Tensor, Tensor)",
        &tcsr_sample);
  m.def("pair_index_build(Tensor src, Tensor dst, int num_nodes) -> (Tensor, Tensor, Tensor)", &pair_index_build);
  m.def("pair_index_contains(Tensor indptr, Tensor indices, Tensor first, Tensor src, Tensor dst, Tensor? before=None, "
        "int before_all=9223372036854775807) -> Tensor",
        &pair_index_contains);
  m.def("negs_hist_rnd(Tensor src, Tensor dst, Tensor t, int lo, int hi, int k, int q, int hist_hi, Tensor indptr, "
        "Tensor indices, Tensor first, Tensor pool, int seed=0, int max_draws=0) -> (Tensor, Tensor, Tensor)",
        &negs_hist_rnd);
  m.def("pairset_insert(Tensor(a!) table, Tensor(b!) status, Tensor src, Tensor dst, Tensor t, int num_nodes) -> ()",
        &pairset_insert);
  m.def("pairset_lookup(Tensor table, Tensor src, Tensor dst, int num_nodes, Tensor? since=None, float? since_all=None) "
        "-> (Tensor, Tensor, Tensor, Tensor)",
        &pairset_lookup);
  m.def("pairset_select(Tensor table, Tensor src, Tensor cand, int num_nodes, Tensor? since=None, float? since_all=None) "
        "-> (Tensor, Tensor)",
        &pairset_select);
  m.def("gemm_f32(Tensor A, Tensor B, Tensor? bias=None, bool trans_a=False, bool trans_b=False) -> Tensor", &gemm_f32);
  // SURVEY §8b's names for the sampler ops (the same functions as ring_sample / ring_insert / ring_reset)
  m.def("sample_recent(Tensor nbr, Tensor e_id, Tensor t, Tensor(a!) assoc, Tensor n_id) -> "
        "(Tensor, Tensor, Tensor, Tensor)",
        &ring_sample);
  m.def("insert_recent(Tensor(a!) nbr, Tensor(b!) e_id, Tensor(c!) t, Tensor src, Tensor dst, Tensor ev_t, "
        "int cur_e_id, Tensor(d!) assoc) -> ()",
        &ring_insert);
  m.def("reset(Tensor(a!) e_id, Tensor(b!) t) -> ()", &ring_reset);
  m.def("msg_agg_last(Tensor msg, Tensor index, Tensor t, int dim_size) -> (Tensor, Tensor)", &msg_agg_last);
  m.def("msg_agg_mean(Tensor msg, Tensor index, int dim_size) -> Tensor", &msg_agg_mean);
  m.def("gru_update(Tensor x, Tensor h, Tensor w_ih, Tensor w_hh, Tensor? b_ih=None, Tensor? b_hh=None, int cell=0) "
        "-> Tensor",
        &gru_update);
  m.def("predictor(Tensor z_src, Tensor z_dst, Tensor w_src, Tensor? b_src, Tensor w_dst, Tensor? b_dst, Tensor w_out, "
        "Tensor b_out, bool sigmoid=True) -> Tensor",
        &predictor);
  m.def("edge_attn_fwd(Tensor q, Tensor k, Tensor v, Tensor? e, Tensor indptr, int heads) -> (Tensor, Tensor)",
        &edge_attn_fwd);
  m.def("edge_attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor? e, Tensor indptr, Tensor alpha, int heads) "
        "-> (Tensor, Tensor, Tensor, Tensor)",
        &edge_attn_bwd);
  m.def("edge_attn_drop_fwd(Tensor q, Tensor k, Tensor v, Tensor? e, Tensor indptr, int heads, float p, int seed, "
        "int stream, Tensor? dst_key, Tensor? edge_key) -> (Tensor, Tensor)",
        &edge_attn_drop_fwd);
  m.def("edge_attn_drop_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor? e, Tensor indptr, Tensor alpha, "
        "int heads, float p, int seed, int stream, Tensor? dst_key, Tensor? edge_key) "
        "-> (Tensor, Tensor, Tensor, Tensor)",
        &edge_attn_drop_bwd);
  // backward ops (tgnx/ops.py wraps them as autograd functions); need[i] = 0 skips gradient i (returned empty)
  m.def("col_sum(Tensor x) -> Tensor", &col_sum);
  m.def("gru_update_bwd(Tensor dh_out, Tensor x, Tensor h, Tensor w_ih, Tensor w_hh, Tensor? b_ih, Tensor? b_hh, "
        "int cell, int[] need) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
        &gru_update_bwd);
  m.def("predictor_topk(Tensor z_src, Tensor z_cand, Tensor w_src, Tensor? b_src, Tensor w_dst, Tensor? b_dst, "
        "Tensor w_out, Tensor b_out, int k, bool sigmoid, bool return_scores) -> (Tensor, Tensor, Tensor)",
        &predictor_topk);
  m.def("predictor_topk_filtered(Tensor z_src, Tensor z_cand, Tensor w_src, Tensor? b_src, Tensor w_dst, "
        "Tensor? b_dst, Tensor w_out, Tensor b_out, int k, bool sigmoid, bool return_scores, Tensor? cand_key, "
        "Tensor? src_key, Tensor? excl_ptr, Tensor? excl_key) -> (Tensor, Tensor, Tensor)",
        &predictor_topk_filtered);
  m.def("embed_knn(Tensor z_q, Tensor z_cand, int metric, int k, bool return_scores, Tensor? cand_key, Tensor? q_key, "
        "Tensor? excl_ptr, Tensor? excl_key) -> (Tensor, Tensor, Tensor)",
        &embed_knn);
  m.def("predictor_topk_lists(Tensor z_src, Tensor z_cand, Tensor w_src, Tensor? b_src, Tensor w_dst, Tensor? b_dst, "
        "Tensor w_out, Tensor b_out, int k, bool sigmoid, bool return_scores, Tensor list_ptr, Tensor list_idx, "
        "int max_len) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
        &predictor_topk_lists);
  m.def("predictor_rank(Tensor z_src, Tensor z_cand, Tensor w_src, Tensor? b_src, Tensor w_dst, Tensor? b_dst, "
        "Tensor w_out, Tensor b_out, Tensor target, int n_count, Tensor? cand_key, Tensor? src_key, Tensor? excl_ptr, "
        "Tensor? excl_key) -> (Tensor, Tensor, Tensor, Tensor)",
        &predictor_rank);
  m.def("predictor_loo(Tensor z, Tensor loo_z, Tensor count, Tensor src_row, Tensor dst_row, Tensor w_src, "
        "Tensor? b_src, Tensor w_dst, Tensor? b_dst, Tensor w_out, Tensor b_out) -> (Tensor, Tensor, Tensor, Tensor)",
        &predictor_loo);
  m.def("predictor_bwd(Tensor dout, Tensor z_src, Tensor z_dst, Tensor w_src, Tensor? b_src, Tensor w_dst, "
        "Tensor? b_dst, Tensor w_out, Tensor b_out, bool sigmoid, int[] need) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
        &predictor_bwd);
  // node property prediction (csrc/tgnx_nodeprop.hip)
  m.def("node_predictor(Tensor z, Tensor w1, Tensor? b1, Tensor w2, Tensor? b2, bool need_h) -> (Tensor, Tensor)",
        &node_predictor);
  m.def("node_predictor_bwd(Tensor dlogits, Tensor z, Tensor h, Tensor w1, Tensor w2, int[] need) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)",
        &node_predictor_bwd);
  m.def("node_loss_ndcg(Tensor logits, Tensor y, Tensor cum, int k, bool need_loss, bool need_grad, bool need_ndcg) "
        "-> (Tensor, Tensor, Tensor, Tensor)",
        &node_loss_ndcg);
  m.def("time_encode(Tensor t, Tensor w, Tensor b) -> Tensor", &time_encode);
  m.def("time_encode_bwd(Tensor dout, Tensor t, Tensor w, Tensor b) -> (Tensor, Tensor)", &time_encode_bwd);
  m.def("time_embedding(Tensor x, Tensor rel_t, Tensor w, Tensor b) -> Tensor", &time_embedding);
  m.def("time_embedding_bwd(Tensor dout, Tensor x, Tensor rel_t, Tensor w, Tensor b, bool need_dx) -> "
        "(Tensor, Tensor, Tensor)",
        &time_embedding_bwd);
  m.def("msg_agg_last_bwd(Tensor dout, Tensor argmax, int n_msg) -> Tensor", &msg_agg_last_bwd);
  m.def("msg_agg_mean_bwd(Tensor dout, Tensor index) -> Tensor", &msg_agg_mean_bwd);
  // device message store (tgnx.nn.TGNMemory / DyRepMemory)
  m.def("memstore_put(Tensor src, Tensor dst, Tensor t, Tensor raw_msg, Tensor sorted, Tensor perm, int start, "
        "Tensor(a!) log_src, Tensor(b!) log_dst, Tensor(c!) log_t, Tensor(d!) log_raw, Tensor(e!) arena, "
        "Tensor(f!) node_tab, Tensor(g!) bad) -> ()",
        &memstore_put);
  m.def("memstore_count(Tensor node_tab, Tensor n_id, Tensor? put_bad=None) -> (Tensor, Tensor)", &memstore_count);
  m.def("memstore_gather(Tensor node_tab, Tensor arena, Tensor log_t, int fill, Tensor n_id, int n_s, int n_d, "
        "Tensor ws) -> (Tensor, Tensor, Tensor, Tensor)",
        &memstore_gather);
  m.def("memstore_build_msg(Tensor slot, int n_s, Tensor log_src, Tensor log_dst, Tensor log_t, Tensor log_raw, "
        "int fill, Tensor memory, Tensor last_update, Tensor w, Tensor b, Tensor? emb=None, Tensor? assoc=None, "
        "Tensor? stamp=None, Tensor? n_id=None, int emb_flags=0) -> (Tensor, Tensor)",
        &memstore_build_msg);
}
