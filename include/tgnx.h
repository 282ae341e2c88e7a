/* libtgnx — MI355X-native (gfx950) TGN temporal link-prediction hot path, C ABI.
 *
 * Every entry point takes plain device pointers, int64 sizes and a HIP stream
 * passed as `void*` (a hipStream_t; NULL = the default stream).  Nothing here
 * allocates: scratch comes from a caller-provided workspace whose size the
 * matching *_ws_bytes() query returns, so a sequence of calls can be captured
 * into a HIP graph.  All launches are asynchronous on `stream`.
 *
 * Return value: TGNX_OK (0) or a negative code; tgnx_last_error() then holds a
 * message (thread-local).  Indices are int64 (the reference's torch.long),
 * times are fp32 (the reference casts t to float32, temporal_dataset.py:42,53).
 *
 * The reference has no native layer: its "FFI" is the Python import seam at
 * pyg-mem-tgn.py:16-25.  Each function below cites the reference code it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer would add.
 */
#ifndef TGNX_H
#define TGNX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGNX_OK 0
#define TGNX_EINVAL (-1)   /* bad argument / shape / capacity */
#define TGNX_EHIP (-2)     /* HIP launch or runtime error */
#define TGNX_ETOOBIG (-3)  /* size beyond what this build supports */

int tgnx_version(void);
const char* tgnx_last_error(void);

/* ------------------------------------------------------------------------
 * Temporal neighbour ring — LastNeighborLoader (neighbor_loader.py:15-109).
 * State: nbr int64[N*K], eid int64[N*K], t fp32[N*K] (row-major [N,K]), newest
 * first in every row; eid < 0 marks an empty slot; assoc int64[N].
 * ------------------------------------------------------------------------ */

/* reset_state (neighbor_loader.py:106-109): eid = -1, t = -1. */
int tgnx_ring_reset(int64_t* eid, float* t, int64_t num_nodes, int32_t size, void* stream);

/* __call__ (neighbor_loader.py:26-50).  Query n_id[q] (any int64 ids < N).
 * Outputs (capacity cap_nodes >= q*(1+K), cap_edges >= q*K):
 *   out_nid[M]          sorted unique of n_id ∪ valid neighbours
 *   out_ei[2*cap_edges] row 0 (local neighbour) at [0,E), row 1 (local centre) at [cap_edges, cap_edges+E)
 *   out_eid[E], out_t[E] in query-row-major, slot order (centre order, then newest first)
 *   assoc[out_nid[i]] = i
 *   counts[0] = M, counts[1] = E   (device int64[2])
 * Workspace: tgnx_ring_sample_ws_bytes(N, q) bytes, zero-filled before the FIRST call
 * (the kernels leave it zeroed again). */
size_t tgnx_ring_sample_ws_bytes(int64_t num_nodes, int64_t q);
int tgnx_ring_sample(const int64_t* nbr, const int64_t* eid, const float* t, int64_t num_nodes,
                     int32_t size, const int64_t* n_id, int64_t q, int64_t* assoc, int64_t* out_nid,
                     int64_t* out_ei, int64_t* out_eid, float* out_t, int64_t cap_nodes,
                     int64_t cap_edges, int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* insert (neighbor_loader.py:52-104) of events (src[i], dst[i], t[i]) with
 * e_id = cur_e_id + i, both directions; keeps the K largest e_id per node
 * (and, as the reference does at :100, the K largest t values separately);
 * assoc[unique touched nodes, sorted] = rank.  B <= tgnx_ring_insert_max_batch().
 * Canonical rule for a node with > K entries in one call: the K newest survive. */
int tgnx_ring_insert_max_batch(void);
int tgnx_ring_insert(int64_t* nbr, int64_t* eid, float* t, int64_t num_nodes, int32_t size,
                     const int64_t* src, const int64_t* dst, const float* ev_t, int64_t B,
                     int64_t cur_e_id, int64_t* assoc, void* stream);

/* ------------------------------------------------------------------------
 * Negative destinations — NegLinkSamplerDest.sample (neg_sampler.py:8-23):
 * uniform over dst_nodes[n_dst], redrawn where equal to pos[i].  Counter-based
 * RNG keyed by (seed, offset + i, attempt): replayable, graph-safe.
 * ------------------------------------------------------------------------ */
int tgnx_neg_sample(const int64_t* dst_nodes, int64_t n_dst, const int64_t* pos, int64_t B,
                    uint64_t seed, uint64_t offset, int64_t* out, void* stream);

/* ------------------------------------------------------------------------
 * Dependency blocks — get_block / dependecyAwareBatch (dependencyGraph.py:8-49),
 * host (CPU, single pass, O(E)) and device versions: per batch of `batch`
 * consecutive events, block = 1 + max(last[src], last[dst]).
 * ------------------------------------------------------------------------ */
int tgnx_block_ids_host(const int64_t* src, const int64_t* dst, int64_t num_events, int64_t batch,
                        int64_t* out);

/* ------------------------------------------------------------------------
 * Kernel probe (measurement only): while enabled, every launch of kernel
 * `kernel_id` (TGNX_K_*) is timed on its launch stream — TGN launches by a pair
 * of hipEvents bound to the dispatch itself (hipExtLaunchKernelGGL start / stop:
 * the kernel's begin / end timestamps, as rocprofv3 --kernel-trace reports),
 * other launches by marker events around them (dispatch included);
 * tgnx_probe_read waits for them and returns the summed duration (ms) and the
 * launch count, then clears.  Off by default.
 * ------------------------------------------------------------------------ */
#define TGNX_K_EDGE_FWD 1       /* tgnn_edge_fwd  */
#define TGNX_K_EDGE_BWD 2       /* tgnn_edge_bwd  */
#define TGNX_K_ASSEMBLE 3
#define TGNX_K_PRED 4
#define TGNX_K_FINISH 5
#define TGNX_K_SEG_FWD 6        /* tgnn_seg_fwd (train and eval) */
#define TGNX_K_ADAM 7
#define TGNX_K_SEG_BWD 8        /* tgnn_seg_bwd */
#define TGNX_K_EDGE_META 9      /* tgnn_edge_meta */
#define TGNX_K_KV 10             /* TGN: kv_reduce ‖ dW_edge ‖ dEnc·W_e launch */
#define TGNX_K_PROJ 11           /* TGN: q / k / v / skip projections launch */
#define TGNX_K_WGRAD3 12         /* TGN: dW_gru ‖ dX_enc ‖ message stores ‖ descriptor snapshot launch */
#define TGNX_K_EXPLAIN 13        /* TGN: tgn_explain_rows (tgnx_tgn_explain's last launch) */
#define TGNX_K_LOO_ROWS 14       /* loo_rows (tgnx_link_predictor_loo's row kernel, after its four GEMMs) */
int tgnx_probe_enable(int32_t kernel_id);
int tgnx_probe_read(double* total_ms, int64_t* launches);
/* Workgroup timeline stamps (diagnostic; measurement only): a library built with -DTGNX_STAMPS records, for
 * wave 0 of every workgroup of the TGN step's kernels, {start, end} (s_memrealtime ticks, 100 MHz), kernel
 * id, block and XCC as 32-byte records into `buf`: 64 shards (by block) of cap / 64 records, shard s at
 * record s * (cap / 64); tgnx_stamps_count returns the fullest shard's count (tools/stamps.py).  buf = NULL
 * stops recording.  Without the flag: tgnx_stamps_set returns TGNX_EINVAL and tgnx_stamps_count -1. */
int tgnx_stamps_set(void* buf, uint32_t cap);
int64_t tgnx_stamps_count(void);


/* ------------------------------------------------------------------------
 * TGNN step — the running reference model (model_utils.py:14-237, 422-697) and
 * its epoch loop (epoch_utils.py:15-318), fused.
 *
 * The per-dependency-block loop of model_utils.py:68-157 is evaluated for all
 * blocks of a batch in one parallel pass: every (row, block) embedding is a
 * segment whose in-edges are the root's ring row (sampled at batch start),
 * its self-loop (ones features, t = 0; epoch_utils.py:246-250) and the
 * intra-batch edges of earlier blocks (model_utils.py:151-157); time_assoc as
 * of block i is reconstructed per source node from the batch's sorted touch
 * list.  EdgeGATConv runs in its exact collapsed form: only
 * U_e = attn_e·W_e, U_{l,r} = attn_{l,r}·W_n reach the output (ft is [N,H,1],
 * :560-563), so the embedding is drop(mem) + (1/H)·Σ_h ft_h.
 *
 * ctl is a device int64[TGNX_CTL_WORDS] (24) control block (see TGNX_CTL_*); every kernel of a
 * step reads the batch geometry from it, so a step can be replayed from a
 * HIP graph.  The model's parameters live in one flat fp32 buffer laid out by
 * tgnx_tgnn_param_layout (names = the reference's state_dict keys).
 * ------------------------------------------------------------------------ */
#define TGNX_CTL_BATCH_START 0  /* offset of the batch's first event in the ev_* arrays */
#define TGNX_CTL_CUR_EID 1      /* e_id of that event (neighbor_loader.py:59) */
#define TGNX_CTL_B 2            /* events in the batch (global batch under DP) */
#define TGNX_CTL_GEN 3          /* node-map generation stamp */
#define TGNX_CTL_ADAM_T 4       /* optimizer step count */
#define TGNX_CTL_S 5            /* segments (rows) assembled */
#define TGNX_CTL_E 6            /* edges assembled (train) */
#define TGNX_CTL_LO 7           /* this rank's event slice [lo, hi) */
#define TGNX_CTL_HI 8
#define TGNX_CTL_SEED 9         /* per-batch RNG seed (dropout) */
#define TGNX_CTL_NB 10          /* batches advanced since the last reset */
#define TGNX_CTL_ERR 11         /* device-side error flags (0 = ok) */
#define TGNX_CTL_LOSS 12        /* (double) running sum of loss * B (epoch_utils.py:310) */
#define TGNX_CTL_SUM_E 13       /* running sum of assembled edges (roofline units) */
#define TGNX_CTL_SUM_S 14       /* running sum of assembled segments */
/* 15: internal (fused-Adam step scalars) */
#define TGNX_CTL_STEP_B 16      /* B of the last trained step (tgnx_tgnn_advance / the resident step's last
                                   launch): what tgnx_tgn_train_update checks, since a pipelined step's
                                   descriptor already holds the NEXT batch when its update runs */
#define TGNX_CTL_APPLY 17       /* TGNN resident world-1 step: Adam step count of the update still to apply
                                   (tgnx_tgnn_train_step_resident defers it to the next step's first launch), 0: none */
#define TGNX_CTL_EVAL_NB 18     /* tgnx_tgn_eval_step_resident: eval batches stepped since the pass began (its own cursor:
                                   a validation pass between two train epochs leaves the train cursor's rule as
                                   tgnx_tgnn_advance has it, NB += 1 per batch) */
#define TGNX_CTL_WORDS 24

#define TGNX_TGNN_NPARAM 15     /* te_w te_b attn_l attn_r attn_e Wn bn We be Ws bs Wd bd Wo bo */

typedef struct {
  int64_t num_nodes;  /* N */
  int32_t ring;       /* K = sampling.neighbor[0] */
  int32_t mem_dim;    /* D = gnn.dim_out (time_dim == D, model_utils.py:18); <= 128 */
  int32_t msg_dim;    /* d (edge-feature width); d + D <= 320 */
  int32_t heads;      /* H = gnn.att_head; 8 */
  int32_t max_batch;  /* capacity of B (global batch); <= 2730 */
  int32_t max_neg;    /* capacity of negatives per event (1 train, K' eval) */
  float feat_drop;    /* 0.6 in the reference (model_utils.py:664) */
  float attn_drop;    /* 0.6 (model_utils.py:665) */
  float lr, beta1, beta2, eps;  /* Adam (model_utils.py:709-710) */
} tgnx_tgnn_config;

typedef struct {
  /* events, indexed like the split arrays; the batch starts at ctl[BATCH_START] */
  const int64_t* ev_src;
  const int64_t* ev_dst;
  const float* ev_t;
  const int64_t* ev_blk;   /* dependency block id of each event */
  const float* ev_msg;     /* [*, d] raw message of each event (intra-batch edge features) */
  int64_t* neg;            /* [*, Kn] negatives, same indexing (train: written by the step) */
  const int64_t* dst_nodes;/* unique destinations for train negatives */
  int64_t n_dst;
  const float* feat;       /* feature table indexed by ring e_id [*, d] (epoch_utils.py:224) */
  int64_t* nbr;            /* ring state (neighbor_loader.py:19-22) */
  int64_t* eid;
  float* rt;
  int64_t* assoc;
  float* time_assoc;       /* [N] model_utils.py:22 */
  const float* memory;     /* [N, D] model_utils.py:270 */
  float* params;           /* flat, tgnx_tgnn_param_layout */
  float* grads;            /* same layout + 1 trailing slot (batch loss) */
  float* adam_m;
  float* adam_v;
  int64_t* ctl;            /* int64[TGNX_CTL_WORDS] */
  float* out_pos;          /* [B] logits (event order in train, block order in eval) */
  float* out_neg;          /* [B*Kn] */
  double* mrr;             /* eval: per-batch MRR, indexed by ctl[NB]-1 */
  void* ws;                /* tgnx_tgnn_ws_bytes(cfg) bytes, zero-filled once */
  void* node_map;          /* int32[4*N], zero-filled once (persistent across steps) */
  float* out_ev;           /* optional (NULL: unused): [num_events, 2] train logits by event row (pos at
                              [2e], neg at [2e + 1]): the epoch's outputs for the AP / AUC display
                              (epoch_utils.py:310-317) without a copy per step */
} tgnx_tgnn_buffers;

int tgnx_tgnn_param_layout(const tgnx_tgnn_config* cfg, int64_t* offsets /* [TGNX_TGNN_NPARAM+1] */);
size_t tgnx_tgnn_ws_bytes(const tgnx_tgnn_config* cfg);
/* Byte offset in ws of the int32[TGNX_MISC_WORDS] per-step diagnostics block: [0] node runs of the
 * ring insert plan, [1] last block id; int64 phase timestamps (wall clock) from [16] in builds with
 * -DTGNX_TIMING.  Measurement only. */
#define TGNX_MISC_WORDS 64
size_t tgnx_tgnn_ws_misc_offset(const tgnx_tgnn_config* cfg);

/* Set up the next batch.  mode 0: explicit (batch_start, B, cur_e_id as given);
 * mode 1: resident (next consecutive batch of `batch` events in [split_lo, split_hi),
 * cur_e_id = the event's global index).  Increments GEN and NB; for train also ADAM_T.
 * rank/world slice the batch's rows for data parallelism. */
int tgnx_tgnn_advance(int64_t* ctl, int32_t mode, int64_t batch_start, int64_t B, int64_t cur_e_id,
                      int64_t split_lo, int64_t split_hi, int64_t batch, int32_t rank, int32_t world,
                      uint64_t base_seed, int32_t train, void* stream);

/* Train step, part 1 (epoch_utils.py:196-303 up to loss.backward): negatives (if gen_neg),
 * assembly, collapsed forward, predictor + BCE, backward; writes grads (+ loss slot).  Also applies
 * the batch's neighbor_loader.insert + time_assoc update (epoch_utils.py:304, model_utils.py:81-83)
 * once the forward has read them (nothing later in the step does). */
int tgnx_tgnn_train_fwd_bwd(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, int32_t gen_neg,
                            int32_t dropout, void* stream);
/* The same for a resident split with the batch cursor folded in (one launch fewer per step):
 * tgnx_tgnn_advance(ctl, mode 1, ..., split_lo, split_hi, batch, rank, world, base_seed, train 1) followed by
 * tgnx_tgnn_train_fwd_bwd(gen_neg 1), as one call.  The step's first launch derives the batch descriptor from the
 * step counter and publishes it; the counter advances in its second launch.  Same results (ctl words included). */
int tgnx_tgnn_train_fwd_bwd_resident(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, int64_t split_lo,
                                     int64_t split_hi, int64_t batch, int32_t rank, int32_t world,
                                     uint64_t base_seed, int32_t dropout, void* stream);
/* World 1: the resident step whole — tgnx_tgnn_train_fwd_bwd_resident (rank 0 of 1) with the update deferred: the
 * step sums its loss and records its update as pending (ctl[TGNX_CTL_APPLY]); the gradient expansion + Adam run in
 * the NEXT call's first launch, beside its batch assembly (8 launches per step, no tgnx_tgnn_train_update).  The
 * parameters therefore lag one step until tgnx_tgnn_apply_pending (call it before reading them; tgnx_tgnn_eval_step
 * applies a pending update itself).  Same results as the separate update, bit for bit. */
int tgnx_tgnn_train_step_resident(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, int64_t split_lo,
                                  int64_t split_hi, int64_t batch, uint64_t base_seed, int32_t dropout, void* stream);
/* Apply the update tgnx_tgnn_train_step_resident left pending, if any (two launches; a no-op on the device when
 * nothing is pending). */
int tgnx_tgnn_apply_pending(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, void* stream);
/* Train step, part 2 (optimizer.step): Adam on the (possibly all-reduced) grads, loss sum. */
int tgnx_tgnn_train_update(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, void* stream);
/* Eval step (epoch_utils.py:28-157): Kn negatives per event, logits in block order,
 * per-batch MRR (TGB rank rule), insert, time_assoc as model_utils.py:77-83 leaves it.
 * tile_quirk = 1 pairs negative row r with source r mod B (model_utils.py:192). */
int tgnx_tgnn_eval_step(const tgnx_tgnn_config* cfg, const tgnx_tgnn_buffers* buf, int32_t Kn,
                        int32_t tile_quirk, void* stream);

/* ---------------------------------------------------------------- dense fp32 GEMM
 * C[M,N] = op(A) op(B) (+ bias[N]) (+ C if accumulate) on v_mfma_f32_16x16x4_f32; K > 256 runs
 * split-K with a fixed-order (deterministic) fixup launch.  op(A)(m,k) = trans_a ? A[k*lda+m] : A[m*lda+k];
 * op(B)(k,n) = trans_b ? B[n*ldb+k] : B[k*ldb+n].  `ws` holds tgnx_gemm_f32_ws_bytes(M,N,K) bytes
 * (split partials).  Used by the TGN memory path (modules: Linear /
 * GRUCell / TransformerConv contractions); exported for tests. */
size_t tgnx_gemm_f32_ws_bytes(int64_t M, int64_t N, int64_t K);
int tgnx_gemm_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, int32_t trans_a, const float* B,
                  int64_t ldb, int32_t trans_b, float* C, int64_t ldc, const float* bias, int32_t accumulate,
                  void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- t-CSR temporal graph
 * TGL's ext_full.npz (indptr int64[N+1], indices int64[nnz], eid int64[nnz], ts fp32[nnz]) that
 * utils.py:73 loads (generated by tgb_gen_graph.py, README.md:5, absent from the reference) and TGL's
 * "recent" neighbour sampler (its C++ sampler_core, README.md:2, also absent).  Rows are ordered by
 * event id (= time order for a chronological stream; *chrono = 0 reports a stream whose t decreases
 * somewhere, for which only the event-id cutoff is meaningful).  Parity unpinned for TGL itself; the
 * event-id cutoff is pinned by the reference's LastNeighborLoader goldens. */
size_t tgnx_tcsr_build_ws_bytes(int64_t num_events, int32_t add_reverse);
/* events (src[e], dst[e], t[e]), e = event id; add_reverse: also the (dst -> src) entry (TGL
 * --add_reverse; LastNeighborLoader inserts both directions).  nnz = E or 2E; nnz < 2^31. */
int tgnx_tcsr_build(const int64_t* src, const int64_t* dst, const float* t, int64_t num_events, int64_t num_nodes,
                    int32_t add_reverse, int64_t* indptr, int64_t* indices, int64_t* eid, float* ts, int32_t* chrono,
                    void* ws, size_t ws_bytes, void* stream);
/* For each root q: the K most recent row entries before the cutoff, newest first, into
 * out_*[q*K + j] (j < out_cnt[q]; the rest nbr = eid = -1, t = -1):
 *   mode 0: eid < cut (cut_eid[q], or cut_eid_all when cut_eid is NULL) — LastNeighborLoader's ring
 *           row at a batch start when cut = the batch's first event id (neighbor_loader.py:52-104);
 *   mode 1: ts < cut_t[q] (TGL: strictly before the root's timestamp).
 * out_cnt may be NULL. */
int tgnx_tcsr_sample(const int64_t* indptr, const int64_t* indices, const int64_t* eid, const float* ts,
                     int64_t num_nodes, int32_t K, const int64_t* roots, int64_t Q, int32_t mode, const int64_t* cut_eid,
                     int64_t cut_eid_all, const float* cut_t, int64_t* out_nbr, int64_t* out_eid, float* out_t,
                     int32_t* out_cnt, void* stream);

/* ---------------------------------------------------------------- pair index and hist_rnd evaluation negatives
 * TGB's link-prediction protocol ranks each positive against `hist_rnd` negatives: destinations the source met
 * before (and is not meeting now) and random destinations that are neither.  TGB generates them offline on the
 * CPU; here they come from a device index of the stream's (source, destination) pairs (DESIGN §3b-12 has the
 * contract, tests/tgb_negs_ref.py restates it).
 *
 * Pair index over rows [0, num_rows) of (src, dst): indptr int64[N+1], indices int64[nnz] (each source's distinct
 * destinations, ascending), first int64[nnz] (the first row at which the pair occurred).  indices / first hold
 * num_rows entries (nnz <= num_rows); *nnz (host, may be NULL) receives nnz = indptr[N] after one synchronisation
 * (offline preprocessing, as tgnx_tcsr_build's *chrono).  Sources must lie in [0, num_nodes), destinations in
 * [0, 2^32), num_nodes <= 2^32, num_rows < 2^31 - 1: TGNX_EINVAL otherwise. */
size_t tgnx_pair_index_build_ws_bytes(int64_t num_rows);
int tgnx_pair_index_build(const int64_t* src, const int64_t* dst, int64_t num_rows, int64_t num_nodes, int64_t* indptr,
                          int64_t* indices, int64_t* first, int64_t* nnz, void* ws, size_t ws_bytes, void* stream);
/* out[i] (one byte, 0 / 1) = the pair (src[i], dst[i]) occurred at a row < before[i] (before_all when before is
 * NULL).  A source outside [0, num_nodes) has seen nothing. */
int tgnx_pair_index_contains(const int64_t* indptr, const int64_t* indices, const int64_t* first, int64_t num_nodes,
                             const int64_t* src, const int64_t* dst, int64_t n, const int64_t* before,
                             int64_t before_all, uint8_t* out, void* stream);
/* k negatives for each event row e of [lo, hi) of a chronological table (t non-decreasing over [lo, hi); t is
 * double[num_events] when t_f64, else float[num_events], and is compared in that type):
 *   P = destinations of the rows of [lo, hi) with e's source and timestamp; Hc = the source's index row restricted
 *   to first < hist_hi; Hn = Hc \ P; X = Hc ∪ P; valid = pool \ X (pool: sorted unique ids below 2^32);
 *   columns [0, k_hist[r]): min(q, |Hn|) historical picks, ascending — all of Hn, or the first q distinct values
 *   outside P of Hc[((hash4(seed, 0x68697374, e, a) >> 11) * |Hc|) >> 53], a = 0, 1, ...;
 *   columns [k_hist[r], k): random picks, ascending — the first distinct values outside X of
 *   pool[((hash4(seed, 0x726E6473, e, a) >> 11) * |pool|) >> 53]; valid[i mod |valid|] when valid is too small;
 *   -1 when it is empty.
 * A draw loop makes at most max_draws draws (0: 16 * its target + 256) and is then filled up with the smallest ids
 * not yet taken.  status int64[4] (device): the first output row with an empty valid set (-1: none), the rows
 * whose historical / random part was filled up, the rows filled cyclically.  k <= 1024 and 0 <= q <= k, else
 * TGNX_EINVAL before any launch.  The result does not depend on the launch geometry. */
size_t tgnx_negs_hist_rnd_ws_bytes(int64_t nnz, int64_t num_rows);
int tgnx_negs_hist_rnd(const int64_t* src, const int64_t* dst, const void* t, int32_t t_f64, int64_t num_events,
                       int64_t lo, int64_t hi, int32_t k, int32_t q, int64_t hist_hi, const int64_t* indptr,
                       const int64_t* indices, const int64_t* first, int64_t num_nodes, int64_t nnz,
                       const int64_t* pool, int64_t n_pool, uint64_t seed, int64_t max_draws, int64_t* out,
                       int32_t* k_hist, int64_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- live pair set (csrc/tgnx_pairset.hip)
 * "Has this source ever interacted with this destination?" for a process that ingests events and retires their
 * rows: an open-addressing hash table of (source, destination) pairs in device memory, updated by one launch per
 * ingested batch.  It names no event rows, so compaction cannot invalidate it (DESIGN §3b-14 has the contract,
 * tests/pairset_ref.py restates it as a dict).
 *
 * table: one device allocation of tgnx_pairset_bytes(capacity) = 20 * capacity bytes, 8-byte aligned; capacity is a
 * power of two >= 64 (else 0 bytes / TGNX_EINVAL):
 *   key     uint64[capacity]  (uint64)src << 32 | dst; the all-ones word is EMPTY
 *   count   uint32[capacity]  occurrences                                             (identity 0)
 *   t_first uint32[capacity]  the smallest stamp as an order-preserving uint32        (identity 0xFFFFFFFF)
 *   t_last  uint32[capacity]  the largest stamp, likewise                             (identity 0)
 * Stamps are the event table's float32 values: bits b (-0.0 taken as 0.0) are stored as ~b when the sign bit is set,
 * else b | 0x80000000, so unsigned integer order is float order and min / max are integer atomics.
 * Home slot = (key * 0x9E3779B97F4A7C15) >> (64 - log2(capacity)) in 64-bit unsigned arithmetic; probing is linear
 * and wraps.  num_nodes must lie in [1, 2^32 - 1] (ids < 2^32 - 1, so no pair is the EMPTY word): TGNX_EINVAL.
 *
 * Every update of a present key is a commutative integer atomic and the value fields hold their identities before
 * a key is published, so the contents are a function of the multiset of inserted events; the slot layout is not,
 * and no output depends on it (tgnx_pairset_export's row order aside: sort by key).  Every loop is bounded: a probe
 * visits at most `capacity` slots, the claim is one 64-bit compare-and-swap per visited slot, and an event that
 * finds no slot is counted and dropped.  No entry point allocates or synchronises with the host.
 *
 * status (device int64[3], zeroed by the caller, accumulated by the kernels): [0] n_keys — keys claimed; [1]
 * n_invalid — events with an id outside [0, num_nodes) or a NaN stamp (never used, never inserted); [2] n_overflow —
 * events that found neither their key nor an EMPTY slot (the table was full; the caller's growth rule prevents it). */
size_t tgnx_pairset_bytes(int64_t capacity);
/* EMPTY keys and the value identities in every slot. */
int tgnx_pairset_init(void* table, int64_t capacity, void* stream);
/* One thread per event (src[i], dst[i], t[i]): claim or find the slot, count += 1, t_first = min, t_last = max. */
int tgnx_pairset_insert(void* table, int64_t capacity, const int64_t* src, const int64_t* dst, const float* t, int64_t n,
                        int64_t num_nodes, int64_t* status, void* stream);
/* tgnx_pairset_insert with given values (tgnx_pairset_export's rows): count[i] in [1, 2^32) is added, t_first[i] /
 * t_last[i] taken with min / max; anything else is counted in n_invalid. */
int tgnx_pairset_import(void* table, int64_t capacity, const int64_t* keys, const int64_t* count, const float* t_first,
                        const float* t_last, int64_t n, int64_t num_nodes, int64_t* status, void* stream);
/* Per query i: out_seen[i] (one byte) = present && t_last >= cut, cut = since[i], or since_all when since is NULL
 * (-inf: no cut; a NaN cut sees nothing); out_count / out_t_first / out_t_last of the pair whatever the cut, and
 * 0 / +inf / -inf for an absent pair.  Any output may be NULL.  An id outside [0, num_nodes) is absent. */
int tgnx_pairset_lookup(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, const int64_t* dst,
                        int64_t n, const float* since, float since_all, uint8_t* out_seen, int64_t* out_count,
                        float* out_t_first, float* out_t_last, void* stream);
/* For every source src[q] the candidates it has met (seen as above; since has Q entries or is NULL), as a ragged
 * (out_ptr int64[Q + 1], out_ids): node ids in candidate order, duplicated candidates kept — the form the link
 * operators take as `exclude`.  Two calls share one workspace: _count fills out_ptr (blocks of one source x 1,024
 * candidates count their hits, one scan), the caller sizes out_ids from out_ptr[Q], _fill with the same arguments
 * writes each block's hits at its offset by ballot / prefix compaction: no cursor, no [Q, C] intermediate, the
 * output bit-identical for every run and grid.  Entries at or beyond out_cap are not written.  Q * ceil(C / 1024)
 * must stay below 2^31 - 1 (0 bytes / TGNX_EINVAL). */
size_t tgnx_pairset_select_ws_bytes(int64_t Q, int64_t C);
int tgnx_pairset_select_count(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, int64_t Q,
                              const int64_t* cand, int64_t C, const float* since, float since_all, int64_t* out_ptr,
                              void* ws, size_t ws_bytes, void* stream);
int tgnx_pairset_select_fill(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, int64_t Q,
                             const int64_t* cand, int64_t C, const float* since, float since_all, int64_t* out_ids,
                             int64_t out_cap, const void* ws, size_t ws_bytes, void* stream);
/* Every live entry of old_table goes into new_table (initialised, any capacity) with its values, except those whose
 * source or destination is flagged in drop_flags (uint8[num_nodes], NULL: none): growth and forgetting in one
 * kernel.  status[0] is set to the new n_keys; status[2] counts entries that did not fit. */
int tgnx_pairset_rehash(const void* old_table, int64_t old_capacity, void* new_table, int64_t new_capacity,
                        const uint8_t* drop_flags, int64_t num_nodes, int64_t* status, void* stream);
/* The live entries, compacted in no particular order: keys (src << 32 | dst), counts, decoded stamps; *out_n
 * (device) = their number.  Rows at or beyond max_out are counted, not written.  The caller sorts by key: the
 * sorted form is the checkpoint. */
int tgnx_pairset_export(const void* table, int64_t capacity, int64_t* out_keys, int64_t* out_count, float* out_t_first,
                        float* out_t_last, int64_t max_out, int64_t* out_n, void* stream);

/* ---------------------------------------------------------------- TGN memory path
 * SURVEY §8 a14–a16 (the PyG TGN of the reference modules/ directory, wired as pyg_model_utils.py:10-36):
 * TGNMemory (modules/memory_module.py:25-215) with IdentityMessage (msg_func.py:12-18) and
 * Last/Mean aggregation (msg_agg.py:15-26), GRUCell memory update, GraphAttentionEmbedding over
 * TransformerConv (emb_module.py:55-73, heads = 2, dropout on the attention), LinkPredictor
 * (decoder.py:12-27, sigmoid output fed to BCE-with-logits as the reference's loop does).
 * The sampler state is the LastNeighborLoader ring above; ctl is the tgnx_tgnn_advance block. */
#define TGNX_TGN_NPARAM 21
/* layers = 2 (SURVEY §8d comment config, "2-hop temporal attention"; the build's extension, no
 * reference parity): the sampler is called again on the 1-hop node set and a second TransformerConv
 * `gnn.conv2` (same shapes as `gnn.conv`) runs on the first one's output; its 9 tensors follow the
 * 21 above in the layout (lin_key w/b, lin_query w/b, lin_value w/b, lin_edge w, lin_skip w/b). */
#define TGNX_TGN_NPARAM2 30
typedef struct {
  int64_t num_nodes;
  int64_t num_events;  /* rows of the event table (e_id space, message-store arena) */
  int32_t ring, mem_dim, msg_dim, heads, max_batch, max_neg;
  int32_t aggr;        /* 0 = LastAggregator, 1 = MeanAggregator */
  float dropout, lr, beta1, beta2, eps;
  int32_t layers;      /* 1 (emb_module.py:55-73) or 2 (2-hop: conv2(conv1(x)) over the 2-hop sample) */
  int32_t updater;     /* memory updater: 0 = GRUCell (TGNMemory memory_module.py:71-72; DyRepMemory 'gru'),
                          1 = RNNCell (DyRepMemory memory_updater_type 'rnn', memory_module.py:256-259):
                          weight_ih [D, Qm], weight_hh [D, D], bias_ih / bias_hh [D] in the same layout slots */
  int32_t emb_in_msg;  /* DyRepMemory (memory_module.py:218-421): bit 0 use_src_emb_in_msg, bit 1
                          use_dst_emb_in_msg (:387-408) — update_state of src ∪ dst builds its messages with the
                          batch's embeddings in place of the memory rows of endpoints in src ∪ dst (train: the
                          train forward's, eval: the eval forward's).  0 = TGNMemory messages.  layers = 1, world 1. */
} tgnx_tgn_config;

typedef struct {
  const int64_t *ev_src, *ev_dst; /* event table [num_events] (e_id rows) */
  const float *ev_t, *ev_msg;     /* [num_events], [num_events, msg_dim] */
  int64_t* neg;                   /* train: [num_events] (written if gen_neg); eval: [num_events, Kn] */
  const int64_t* dst_nodes;
  int64_t n_dst;
  int64_t *nbr, *eid;             /* LastNeighborLoader ring [N,K] */
  float* rt;
  int64_t* assoc;                 /* [N] */
  float* memory;                  /* TGNMemory.memory [N, mem_dim] */
  int64_t* last_update;           /* TGNMemory.last_update [N] */
  int64_t* store;                 /* message stores: tgnx_tgn_store_words(cfg) int64, zero-filled once */
  int32_t* node_gen;              /* int32[N], zero-filled once */
  float *params, *grads, *adam_m, *adam_v; /* flat, tgnx_tgn_param_layout (+1 loss slot in grads) */
  int64_t* ctl;                   /* int64[TGNX_CTL_WORDS] */
  float *out_pos, *out_neg;       /* train: [B] sigmoid outputs; eval: [B], [B, Kn] */
  double* mrr;                    /* eval: per-event reciprocal ranks of the last batch [B] */
  void* ws;                       /* tgnx_tgn_ws_bytes(cfg), zero-filled once */
  float* xrows;                   /* data parallel (ctl world > 1): [xcap, TGNX_TGN_ROW(mem_dim)] rows this
                                     rank's step updated, exchanged after the step; NULL at
                                     world 1 */
  int64_t xcap;                   /* >= 2 * ceil(max_batch / world) */
  float* out_ev;                  /* optional (NULL: unused): [num_events, 2] train outputs by event row —
                                     sigmoid(pos), sigmoid(neg) of event e at [2e], [2e + 1] — so that an
                                     epoch of replayed steps leaves every batch's outputs for the AP / AUC
                                     display (pyg_epoch_utils.py:139-147) without a copy per step */
  const void* plan_table;         /* optional (NULL: unused): the plan table tgnx_tgn_plan_table built for the
                                     split / batch the resident parity-set steps run (tgnx_tgn_train_step_pp,
                                     tgnx_tgn_train_fwd_bwd_pp); they then read every batch's ring-insert and
                                     message-store plans from it and their scan is the node-set walk alone.
                                     Other calls ignore it.  Must be the table tgnx_tgn_plan_table built for
                                     the steps' split_lo / split_hi / batch and this config's max_batch: the
                                     library records that when it builds the table and the steps refuse
                                     (TGNX_EINVAL) a table it did not build or one built for another split. */
  int32_t flags;                  /* TGNX_TGN_* bits below (0: defaults) */
} tgnx_tgn_buffers;
/* tgnx_tgn_buffers.flags: the steps with Adam fused into the gradient writers (tgnx_tgn_train_step*, world 1)
 * update parameters and moments without storing the gradient in buf->grads (the batch loss slot
 * grads[P] is still written); for loops that never read the gradients (the benchmark, the drop-in train()) */
#define TGNX_TGN_NO_GRAD_STORE 1
/* tgnx_tgn_train_step_pp at 1 hop with LastAggregator, the GRU cell and TGNMemory messages gathers the NEXT batch's
 * parameter-free message rows (tgn_agg_emit's root / edge records, msg and memory columns, accumulator zeroing)
 * inside its fixup launch, and writes memory / last_update one launch earlier; the next step then starts with the
 * short tgn_enc_fill launch (the time-encoding columns from its own te_w / te_b) instead of tgn_agg_emit.  The
 * message columns of the next batch are therefore copied out of the memory table before the step returns: a
 * caller that rewrites memory / last_update / the stores between two prefetched steps must issue the next step
 * with prefetched = 0.  This bit keeps the step on tgn_agg_emit (every other step form always is). */
#define TGNX_TGN_NO_GATHER_AHEAD 2
/* exchanged memory row, all fields floats holding exact integers so that the row survives a SUM exchange
 * (one all-reduce over [gradients | every rank's row slots, zero but the sender's] is the all-gather):
 * node (-1 = unused slot; num_nodes < 2^24), last_update bits 0-23, 24-47, 48-63, memory[D] */
#define TGNX_TGN_ROW(D) ((D) + 4)

int tgnx_tgn_param_layout(const tgnx_tgn_config* cfg,
                          int64_t* offsets /* [TGNX_TGN_NPARAM+1], layers = 2: [TGNX_TGN_NPARAM2+1] */);
size_t tgnx_tgn_ws_bytes(const tgnx_tgn_config* cfg);
size_t tgnx_tgn_store_words(const tgnx_tgn_config* cfg);
/* The ring-insert plan (neighbor_loader.py:52-104: the batch's (node, event, direction) entries in node
 * order, newest first, runs per node) and the message-store plan (memory_module.py:180-191: stable per
 * (node, direction), runs) of every batch of a resident split [split_lo, split_hi) in batches of `batch`
 * (the global batch under data parallelism): a function of the event table alone, so one launch per
 * binding builds what each step's scan would otherwise sort again.  Table: tgnx_tgn_plan_table_bytes bytes
 * (a 64-B header + one slot per batch, sized by max_batch: 2 max_batch entries of 20 B each, i.e. about 40 B
 * per event of the split when batch = max_batch — ~6 MB for the tgbl-wiki train split, ~1.3 GB for a
 * tgbl-comment-sized one of 31M events); hand it to the resident parity-set steps as buf->plan_table. */
size_t tgnx_tgn_plan_table_bytes(const tgnx_tgn_config* cfg, int64_t split_lo, int64_t split_hi, int64_t batch);
int tgnx_tgn_plan_table(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo, int64_t split_hi,
                        int64_t batch, void* table, size_t table_bytes, void* stream);
/* Forget what `table` was built for (the library keeps, per table address, the split / batch it serves, and the
 * steps refuse a table built for another): call before freeing a plan table, so a later allocation at the same
 * address is not taken for it.  A (re)build forgets first and records only after its launch was issued. */
int tgnx_tgn_plan_table_release(const void* table);
/* memory = 0, last_update = 0, message stores empty (memory_module.py:106-110). */
int tgnx_tgn_reset_state(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, void* stream);
/* Train batch, part 1 (the canonical loop pyg_epoch_utils.py:106-137 carries commented out): negatives
 * (gen_neg), sampler, memory(n_id) with the GRU update of every sampled node, embedding,
 * link prediction, BCE, backward; then update_state (memory / last_update of src ∪ dst, message
 * stores) and the ring insert.  Writes grads (+ loss slot).
 * Data parallel (ctl rank / world from tgnx_tgnn_advance): the roots, GRU, embedding, prediction and
 * loss cover this rank's event slice only (grads are its share of the global-batch mean; sum them
 * across ranks); message stores and the ring insert replay the whole global batch (replicated);
 * the memory rows this rank updated are packed into buf->xrows for the all-gather. */
int tgnx_tgn_train_fwd_bwd(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int32_t gen_neg,
                           int32_t dropout, void* stream);
/* Train batch in one call at world 1: tgnx_tgn_train_fwd_bwd with Adam folded into the gradient writers
 * (every gradient element's writer also updates its parameter / adam_m / adam_v), equal to fwd_bwd +
 * tgnx_tgn_train_update (grads are still written).  Refused with xrows set (data parallel). */
int tgnx_tgn_train_step(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int32_t gen_neg, int32_t dropout,
                        void* stream);
/* tgnx_tgn_train_step of the next batch of a resident split, with the batch cursor folded in: the
 * same as tgnx_tgnn_advance(ctl, mode 1, ..., split_lo, split_hi, batch, rank, world, base_seed,
 * train 1) followed by tgnx_tgn_train_step(gen_neg 1), one launch fewer.  World 1 only (Adam is folded
 * in as well; world > 1 is refused), split_hi <= num_events.
 * ctl words, in stream order: the step's second launch (the scan) writes the batch descriptor
 * (BATCH_START, B, CUR_EID, LO, HI, SEED) from the unchanged counters; the step's LAST launch advances NB,
 * GEN and (when B > 0) ADAM_T.  So once the call's work has completed, ctl equals what advance + step leave; between
 * the two (e.g. a kernel of the caller's own, enqueued in between) the counters still hold the previous
 * step's values, whereas tgnx_tgnn_advance has already advanced them. */
int tgnx_tgn_train_step_resident(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                 int64_t split_hi, int64_t batch, int32_t rank, int32_t world, uint64_t base_seed,
                                 int32_t dropout, void* stream);
/* tgnx_tgn_train_step_resident (world 1) pipelined across steps: the step marks the NEXT batch of the split
 * inside its predictor launch (its ring insert now runs beside the GRU, before that) and scans it after its
 * own last launch, so the next pipelined call starts at the message aggregation: two launches fewer per
 * step on the critical path.  prefetched = 1: the previous call on these buffers was a pipelined step with
 * the same split / batch / seed and nothing else ran on them since; prefetched = 0: mark + scan this batch
 * first (the first step, or after any other call: eval, flush, reset, another train form, a new cursor).
 * Results equal tgnx_tgn_train_step_resident's step for step (same batches, negatives, dropout streams).
 * ctl after the call: NB / GEN / ADAM_T advanced as for the resident step; the batch descriptor words
 * (BATCH_START .. SEED) and SUM_E / SUM_S already describe / include the NEXT batch, and neg[] holds the
 * next batch's negatives.  Test: tests/test_gpu_tgn.py (pipelined vs resident). */
int tgnx_tgn_train_step_pipelined(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                  int64_t split_hi, int64_t batch, uint64_t base_seed, int32_t dropout,
                                  int32_t prefetched, void* stream);
/* tgnx_tgn_train_step_pipelined with two parities of the scan's per-batch outputs (sorted node / centre sets,
 * edge offsets, update list, insert / store plans, counts) in the workspace: a step reads set `parity`
 * while the next batch is marked in its predictor launch and scanned into set 1 - parity inside its k / v
 * reduction launch, so its last launch (split-K sums, Adam, memory update) no longer waits for the scan.
 * Alternate parity 0, 1, 0, ... across consecutive calls (two HIP graphs); prefetched as for
 * tgnx_tgn_train_step_pipelined (prefetched = 0 marks + scans this batch into set `parity` first).  A step
 * whose set holds another batch (wrong parity) sets ctl[ERR] bit 16 and computes nothing after its first
 * launch.  World 1, 1 or 2 hops (2 hops: the root level's sets are doubled too, and the next batch's node-set
 * walk rides in the dW_cell launch); other calls use set 0 and scan for themselves.  Results equal
 * tgnx_tgn_train_step_pipelined's step for step.  Test: tests/test_gpu_tgn.py (pp vs resident, both hops). */
int tgnx_tgn_train_step_pp(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                           int64_t split_hi, int64_t batch, uint64_t base_seed, int32_t dropout, int32_t prefetched,
                           int32_t parity, void* stream);
/* Data parallel form: tgnx_tgn_train_fwd_bwd with the folded cursor (the exchange, tgnx_tgn_apply_rows and
 * tgnx_tgn_train_update follow).  ctl words as for tgnx_tgn_train_step_resident: the descriptor is written
 * by the first launch, NB / GEN / ADAM_T advance in the last launch of THIS call, so they have advanced
 * by the time the exchange and tgnx_tgn_train_update (which reads ADAM_T) run — the same values the
 * advance + fwd_bwd path gives them.  Test: tests/test_gpu_tgn_dp.py (per rank, folded vs advance +
 * fwd_bwd). */
int tgnx_tgn_train_fwd_bwd_resident(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                    int64_t split_hi, int64_t batch, int32_t rank, int32_t world,
                                    uint64_t base_seed, int32_t dropout, void* stream);
/* tgnx_tgn_train_fwd_bwd_resident pipelined across steps, as tgnx_tgn_train_step_pipelined (world >= 1;
 * Adam is not folded in): the next batch (this rank's slice) is marked inside the k / v reduction launch and
 * scanned after this call's last launch, so the next call starts at the message aggregation.  The exchange
 * and tgnx_tgn_apply_rows_update follow each call (that update reads STEP_B, not B: the descriptor words
 * already describe the next batch).  prefetched as for tgnx_tgn_train_step_pipelined.  Per rank, results
 * equal tgnx_tgn_train_fwd_bwd_resident's step for step.  Test: tests/test_gpu_tgn_dp.py. */
int tgnx_tgn_train_fwd_bwd_pipelined(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                     int64_t split_hi, int64_t batch, int32_t rank, int32_t world,
                                     uint64_t base_seed, int32_t dropout, int32_t prefetched, void* stream);
/* tgnx_tgn_train_fwd_bwd_pipelined without its last launch (the next batch's scan), and that scan alone:
 * fwd_bwd_split, then the exchange started asynchronously, tgnx_tgn_scan_next on the compute stream while
 * the collective runs (the scan touches neither the exchange buffer nor what the update writes), then
 * tgnx_tgn_apply_rows_update after the exchange — the same results as the pipelined call. */
int tgnx_tgn_train_fwd_bwd_split(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                 int64_t split_hi, int64_t batch, int32_t rank, int32_t world, uint64_t base_seed,
                                 int32_t dropout, int32_t prefetched, void* stream);
int tgnx_tgn_scan_next(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo, int64_t split_hi,
                       int64_t batch, int32_t rank, int32_t world, uint64_t base_seed, void* stream);
/* The data-parallel step on the parity-set design of tgnx_tgn_train_step_pp (world >= 1, 1 or 2 hops, Adam not
 * folded in): the next batch (this rank's slice) is marked in the predictor launch and scanned into set
 * 1 - parity inside the dW_cell launch; the last launch writes the gradients, packs this rank's updated
 * memory rows into buf->xrows, advances the counters and writes the next descriptor.  One step is this
 * call, then the exchange (the all-reduce of [gradients | row slots]), then tgnx_tgn_apply_rows_update —
 * which this call runs FIRST when apply_prev = 1 (rows / nrows: the whole exchanged row block), so that a
 * step is one graph [apply(k-1) ‖ step k] plus one collective.  apply_prev must be 1 exactly when the
 * previous call's exchange has not yet been applied.  prefetched / parity as tgnx_tgn_train_step_pp.
 * Test: tests/test_gpu_tgn_dp.py (per rank against the split pipelined step) and tests/test_gpu_tgn_dp_worlds.py. */
int tgnx_tgn_train_fwd_bwd_pp(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                              int64_t split_hi, int64_t batch, int32_t rank, int32_t world, uint64_t base_seed,
                              int32_t dropout, int32_t prefetched, int32_t parity, int32_t apply_prev, float* rows,
                              int64_t nrows, void* stream);
/* The launch plan of a train step (host only: no device, no buffers; as tgnx_block_ids_host).  Every train entry
 * point above decides in one place which launches it issues, how big they are and what rides in them; this returns
 * those decisions, so that they can be pinned without a GPU (tests/test_step_plan_cpu.py).  The mode as the entry
 * points spell it: fuse_adam (tgnx_tgn_train_step*), world (0: no device cursor; >= 1: a resident step of that
 * world), prefetch (TGNX_TGN_PREFETCH_*), caller_scans (tgnx_tgn_train_fwd_bwd_split), parity (-1: one scan-output
 * set; 0 / 1: _pp).  xrows / plan_table: that buffer is set; flags: tgnx_tgn_buffers.flags.  out: one record per
 * launch label, in launch order (TGNX_TGN_STEP_LAUNCHES of them); a launch that is not issued has only its label.
 * grid / block in workgroups / threads, lds = the dynamic LDS bytes of the launch, kernel = which instance the label
 * launches (TGNX_TGN_AGG_*, _PRED_*, _ATTB_*, _FIXUP_*; tgn_gru_edge: 1 = with conv2's lin_edge; tgn_wgrad_dz0 /
 * tgn_wgrad3: 1 = the launch carries the next batch's ScanJob; else 0). */
#define TGNX_TGN_STEP_LAUNCHES 21
#define TGNX_TGN_STEP_LABELS                                                                                        \
  "tgn_mark", "tgn_scan", "tgn_gather", "tgn_agg_emit", "tgn_gru_edge", "tgn_proj", "tgn_attn_fwd", "tgn_proj2",    \
      "tgn_attn_fwd2", "tgn_pred_train", "tgn_emb_update", "tgn_emb_update_gru", "tgn_attn_bwd2", "tgn_kv_reduce2", \
      "tgn_dh1", "tgn_attn_bwd", "tgn_wgrad_dz0", "tgn_wgrad3", "tgn_scan_early", "tgn_fixup_update", "tgn_scan_next"
#define TGNX_TGN_PREFETCH_PLAIN 0    /* not pipelined */
#define TGNX_TGN_PREFETCH_PREPARED 1 /* pipelined, prefetched = 1 */
#define TGNX_TGN_PREFETCH_FIRST 2    /* pipelined, prefetched = 0: the step prepares its own batch first */
#define TGNX_TGN_AGG_ENC_FILL 0 /* tgn_enc_fill (gather-ahead) */
#define TGNX_TGN_AGG_LAST 1     /* tgn_agg_emit<0> */
#define TGNX_TGN_AGG_MEAN 2     /* tgn_agg_emit<1> (msg_dim <= 192) */
#define TGNX_TGN_AGG_ANY 3      /* tgn_agg_emit<-1> */
#define TGNX_TGN_PRED_RING10 0 /* tgn_pred_train<true, 10> */
#define TGNX_TGN_PRED_RING 1   /* tgn_pred_train<true, 16> */
#define TGNX_TGN_PRED_2HOP 2   /* tgn_pred_train<false> */
#define TGNX_TGN_ATTB_EB10_REP 0 /* tgn_attn_bwd<10, 4> */
#define TGNX_TGN_ATTB_EB16_REP 1 /* tgn_attn_bwd<16, 4> */
#define TGNX_TGN_ATTB_EB10 2     /* tgn_attn_bwd<10, 1> */
#define TGNX_TGN_ATTB_EB16 3     /* tgn_attn_bwd<16, 1> */
#define TGNX_TGN_FIXUP_1HOP 0   /* TrainTail<false>, 4 weight gradients */
#define TGNX_TGN_FIXUP_GATHER 1 /* TrainTail<true>: the next batch's gather rides */
#define TGNX_TGN_FIXUP_2HOP 2   /* TrainTail<false>, 6 weight gradients */
typedef struct tgnx_tgn_launch {
  int32_t label, issued, grid, block, lds, kernel;
} tgnx_tgn_launch;
int tgnx_tgn_step_plan(const tgnx_tgn_config* cfg, int32_t fuse_adam, int32_t world, int32_t prefetch,
                       int32_t caller_scans, int32_t parity, int32_t xrows, int32_t plan_table, int32_t flags,
                       tgnx_tgn_launch* out);
/* tgnx_tgn_apply_rows + tgnx_tgn_train_update in one launch (data parallel, after the exchange). */
int tgnx_tgn_apply_rows_update(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, float* rows, int64_t nrows,
                               void* stream);
/* Data parallel: write the exchanged rows of every rank (rows [nrows, TGNX_TGN_ROW(mem_dim)], slots
 * with node -1 skipped) into memory / last_update, then zero `rows` (ready for the next summing
 * exchange).  Ranks that updated the same node computed the same row (same replicated inputs), so the
 * order does not matter. */
int tgnx_tgn_apply_rows(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, float* rows, int64_t nrows,
                        void* stream);
/* Train batch, part 2: Adam on the (possibly all-reduced) grads, loss sum; nothing when the step's batch
 * (ctl STEP_B) was empty. */
int tgnx_tgn_train_update(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, void* stream);
/* Eval batch (TGB tgbl link prediction): every event's [pos, Kn negatives] scored with the
 * batch-start memory and ring, per-event reciprocal rank in buf->mrr, then update_state in eval
 * order (store, then GRU update) and the ring insert. */
int tgnx_tgn_eval_step(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int32_t Kn, void* stream);
/* The resident form of tgnx_tgn_eval_step: a validation / test pass over events [split_lo, split_hi) in batches of
 * `batch` with no host work between batches.  The batch comes from the device cursor ctl[TGNX_CTL_EVAL_NB] (batch nb
 * = events [split_lo + nb * batch, ...), the last one partial, a step past the end a no-op with B = 0), which this
 * call advances together with GEN / NB (as tgnx_tgnn_advance with train = 0 does; ADAM_T untouched); set the cursor
 * word to 0 to begin a pass.  No argument changes from batch to batch, so one captured HIP graph serves the split.
 * buf->neg is the split's negatives table int64 [split_hi - split_lo, Kn] (row e - split_lo = event e's negatives);
 * rr_ev is double [split_hi - split_lo]: event e's reciprocal rank is written to rr_ev[e - split_lo] (buf->mrr[i],
 * out_pos / out_neg hold the last batch, as after tgnx_tgn_eval_step).  rank / world / base_seed fill the
 * descriptor's LO / HI / SEED words only: every rank evaluates the whole batch.
 * The marking is deduplicated: each distinct candidate node's ring row is walked once per batch instead of once per
 * candidate slot (two launches, tgn_eval_claim + tgn_mark_eval, for tgn_mark<false>); the sampled sets, and every
 * launch after the scan, are those of tgnx_tgn_eval_step, and so are the results, bit for bit.
 * Test: tests/test_gpu_tgn_eval_resident.py (against the per-batch step, the oracle at 999 negatives, and the
 * duplicate-candidate cases on both bitmap branches). */
int tgnx_tgn_eval_step_resident(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t split_lo,
                                int64_t split_hi, int64_t batch, int32_t Kn, int32_t rank, int32_t world,
                                uint64_t base_seed, double* rr_ev, void* stream);
/* Read-only inference: the embeddings of an explicit node list at the current stream state — out_z[i] [mem_dim] is
 * the embedding of nodes[i] as tgnx_tgn_eval_step computes it before scoring: memory / last_update rows as stored
 * (eval mode, memory_module.py:116-124; nothing is flushed: after train steps call tgnx_tgn_flush first), the ring
 * sampled for the node set (twice at layers = 2), GraphAttentionEmbedding.  The launches are the eval step's up to
 * tgn_attn_fwd (tgn_attn_fwd2), with the roots taken from `nodes` (tgn_embed_claim / tgn_embed_mark), the scan's
 * node-set walk alone (no batch, so no insert / store plans), and one gather of the roots' rows into out_z; no
 * scoring, no update_state, no ring insert.  Duplicates are allowed.  A node outside [0, num_nodes) is never used as
 * an index: its row is zero-filled and it is counted into *n_invalid (a device int64 the caller zeroes; may be NULL).
 * n <= tgnx_tgn_embed_max_nodes(cfg) = the eval root capacity min(num_nodes, max_batch * (2 + max_neg)); more is
 * TGNX_EINVAL (the caller chunks: calls are independent).  n = 0 does nothing.
 * Read-only: memory, last_update, the message stores, the ring, node_gen, parameters, gradients and Adam moments are
 * untouched, and so is every ctl word but two — TGNX_CTL_GEN advances by one per call (node_gen stamps are compared
 * to it: it stays monotonic, and no stamp equals the new value, so the update list is empty) and TGNX_CTL_ERR takes
 * the capacity-overflow bit the scan would set.  The kernels read the batch geometry from a private copy of ctl in
 * the workspace (B = n, GEN = the new value; the scan's SUM_E / SUM_S additions land there); on a nonzero ERR the
 * call computes nothing and zero-fills out_z.  assoc and the workspace (sampled sets, bitmaps, the scan-output set 0)
 * are scratch as for every step: a pipelined / parity-set train step after it must run with prefetched = 0. */
int64_t tgnx_tgn_embed_max_nodes(const tgnx_tgn_config* cfg);
int tgnx_tgn_embed(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, const int64_t* nodes, int64_t n,
                   float* out_z /* [n, mem_dim] */, int64_t* n_invalid /* device, caller-zeroed, may be NULL */,
                   void* stream);
/* Why a link score is what it is: tgnx_tgn_embed for the listed nodes with, per node, the ring slots
 * its embedding attended over, the attention weights, and the embedding recomputed with a slot (or a neighbour) absent.
 * The launches are tgnx_tgn_embed's with tgn_explain_rows in tgn_embed_gather's place: the same claim / mark /
 * inference forward, the same private ctl copy and ERR OR-back, the same capacity (n <= tgnx_tgn_embed_max_nodes), the
 * same read-only guarantees (GEN advances by one; ERR may take the overflow bit, and every output is then as for an
 * invalid id), ids outside [0, num_nodes) counted into *n_invalid and never used as an index.  K = cfg->ring,
 * D = cfg->mem_dim.  Per listed node i, whose root level samples the ne valid slots of its ring row in slot order:
 *   z[i, D]            the embedding, bit for bit tgnx_tgn_embed's row;
 *   count[i]           ne;
 *   slot_eid[i, K], slot_nbr[i, K]   the slot's event row and the neighbour's node id, -1 past ne;
 *   alpha[i, K, 2]     the root level's eval attention per head (a = q · (k + e) / sqrt(C), max subtracted, + 1e-16 in
 *                      the denominator), 0 past ne;
 *   loo_z[i, K, D]     row j: the embedding with the slots S_j absent — S_j = {j} (TGNX_EXPLAIN_SLOT) or every slot
 *                      u with slot_nbr[u] == slot_nbr[j] (TGNX_EXPLAIN_NEIGHBOUR) — recomputed from the scores (max,
 *                      exponentials and denominator over the remaining slots, summed in slot order, + the skip row),
 *                      not derived from z by division; an empty remainder gives the skip row, the embedding of a node
 *                      without edges.  Rows j >= ne are zero.
 * An invalid id: zero rows, count 0, slots -1.  loo_z may be NULL (the attention alone).  At layers = 2 alpha is the
 * root level's (conv2 over the node's own ring row) and loo_z must be NULL: removing an edge there also changes the
 * node's own hop-1 row, hence the second hop's query and skip; a non-NULL loo_z is TGNX_EINVAL before any launch.
 * No atomics in tgn_explain_rows, every loop bounded by the ring width; a row does not depend on the grid or on how a
 * node list is chunked.  No host synchronisation, no allocation.
 * Test: tests/test_gpu_tgn_explain.py (against the oracle with the ring slots masked out of its sampler). */
#define TGNX_EXPLAIN_SLOT 0
#define TGNX_EXPLAIN_NEIGHBOUR 1
int tgnx_tgn_explain(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, const int64_t* nodes, int64_t n,
                     int32_t mode, float* z /* [n, D] */, int32_t* count /* [n] */, int64_t* slot_eid /* [n, K] */,
                     int64_t* slot_nbr /* [n, K] */, float* alpha /* [n, K, 2] */,
                     float* loo_z /* [n, K, D], may be NULL */, int64_t* n_invalid /* device, may be NULL */,
                     void* stream);
/* Score-free ingestion: the state update of tgnx_tgn_eval_step for the batch ctl describes (as after
 * tgnx_tgnn_advance(..., train = 0)), without negatives and without the forward that scores them — update_state in
 * eval order (memory_module.py:126-138 with training == False: store the batch's messages, aggregate and run the
 * memory updater over src ∪ dst, write memory and last_update) and the ring insert (neighbor_loader.insert).
 * buf->neg, out_pos, out_neg and mrr are not read and may be NULL.  Afterwards memory, last_update, the stores, the
 * ring, node_gen and the ctl words an eval step moves (none beyond what the advance set; SUM_E / SUM_S grow by 0 and
 * by |src ∪ dst|, not by the eval step's sample) are what tgnx_tgn_eval_step leaves for the same batch with any
 * negatives.
 * emb_in_msg == 0, 6 launches at either `layers` (the eval step has 11 at 1 hop): tgn_observe_mark (one thread per
 * endpoint: node_gen stamp, kval = 0, centre + node bit; no ring row is read, no neighbour or candidate is marked),
 * tgn_scan (update list = centres = nodes, and the insert / store plans), tgn_update (stores + ring), the aggregation
 * and the updater GEMM of the update list, tgn_update (memory write).  No edge / projection GEMM, no attention, no
 * predictor, no score: no work proportional to Kn or to the ring width.
 * emb_in_msg != 0 (DyRep embedding messages, 1 hop): the stored messages carry the eval forward's embeddings of
 * src ∪ dst, so after tgn_observe_mark the eval launches up to tgn_attn_fwd run for the 2B endpoint roots (tgn_mark
 * with no negative slots), then the same update; still no predictor or score launch.
 * B == 0 launches work that returns at once and changes no state (the marking clears the scan's counts, so no
 * earlier batch's update runs again).  A batch beyond max_batch or the event table, or an endpoint outside
 * [0, num_nodes), sets TGNX_CTL_ERR bit 4 and the step does nothing further.  No host synchronisation, no allocation.
 * One device only (no row exchange).  assoc and the workspace are scratch as for every step: a pipelined / parity-set
 * train step after it must run with prefetched = 0.
 * Test: tests/test_gpu_tgn_observe.py (against the eval step bit for bit, and against the oracle's update_state). */
int tgnx_tgn_observe_step(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, void* stream);

/* The embedding table (csrc/tgnx_embtab.hip): a materialised table[num_nodes, mem_dim] of what
 * tgnx_tgn_embed returns, kept current by recomputing only the rows a batch made stale.  In eval mode the embedding of
 * v is a function of v's memory / last_update and ring row, of the memory / last_update of the nodes in that row (and of
 * their ring rows at layers = 2) and of immutable event rows; no query time enters.  With T the nodes whose memory,
 * last_update or ring row was written since the table was current (the endpoints of every observed / evaluated batch)
 * and ring(v) the entries of v's ring row with e_id >= 0 (reset_state leaves stale ids under e_id = -1):
 *   D1 = { v : ring(v) meets T },  D2 = { v : ring(v) meets T | D1 },
 *   stale = T | D1 at layers = 1,  T | D1 | D2 at layers = 2,
 * evaluated on the ring as it stands when the list is made (an untouched node's row is what it was, a touched node is
 * in T itself).  flags: uint8 planes [3][N] for T, D1, D2 (plane p at flags + p * N, N the node count of the call; a
 * caller whose N grows re-lays them), zero when nothing is stale.  Every flag write is an idempotent plain store: no
 * atomics, no read-modify-write of a shared byte.  One device only: the calls that take buf refuse a data-parallel
 * engine's buffers (buf->xrows set) with TGNX_EINVAL.  No host synchronisation, no allocation.
 * Test: tests/test_gpu_embtab.py (ids against a numpy restatement of the rule, rows against the oracle).
 *
 * tgnx_embtab_touch (1 launch): T[src[i]] = T[dst[i]] = 1 for i < B, one thread per endpoint; an id outside [0, N) is
 * skipped.  B = 0 does nothing.
 * tgnx_embtab_expand (1 launch, 2 at layers = 2): walks the ring [N, K] flat over (node, slot), reads T and writes D1,
 * then reads T | D1 and writes D2; no pass reads the plane it writes.  D1 / D2 must be zero on entry (the list call
 * leaves them so).
 * tgnx_embtab_list (3 launches): out_ids = the ascending ids with any plane set (capacity N), *out_count (device
 * int64) their number; all three planes are cleared.  The order comes from a fixed-order scan (wave ballot / popcount,
 * then a scan of the workgroups' counts), so the list is run-to-run identical.  ws: tgnx_embtab_list_ws_bytes(N)
 * bytes, 4-B aligned, not zeroed.  N >= 2^31: TGNX_ETOOBIG.
 * tgnx_tgn_embed_into: tgnx_tgn_embed whose last launch writes the row of nodes[i] to table[nodes[i]] instead of
 * out_z[i]: same launches, same capacity rule (n <= tgnx_tgn_embed_max_nodes), same private control-block copy, same
 * read-only guarantees (GEN advances, ERR may take the overflow bit, and the listed rows are then zero-filled).  nodes
 * must hold no duplicates (two waves would write one row; equal values, but unordered) — the list call's output has
 * none; an id outside [0, num_nodes) writes nothing.  table has at least num_nodes rows. */
int tgnx_embtab_touch(const int64_t* src, const int64_t* dst, int64_t B, int64_t N, uint8_t* flags, void* stream);
int tgnx_embtab_expand(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, uint8_t* flags, void* stream);
size_t tgnx_embtab_list_ws_bytes(int64_t N);
int tgnx_embtab_list(uint8_t* flags, int64_t N, int32_t layers, int64_t* out_ids, int64_t* out_count, void* ws,
                     size_t ws_bytes, void* stream);
int tgnx_tgn_embed_into(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, const int64_t* nodes, int64_t n,
                        float* table /* [>= num_nodes, mem_dim] */, void* stream);

/* Event-table compaction (csrc/tgnx_compact.hip): retire every row of the event table that nothing
 * references and renumber the survivors order-preservingly (new id = rank among the live rows).  A row e of the
 * num_events valid rows (cfg->num_events is the capacity) is live when a ring slot with nbr != -1 holds it, when a
 * node's s- or d-store run holds it, or when e >= upto.  Two calls, because the caller sizes the new allocations
 * from one number in between; ws is tgnx_tgn_compact_ws_bytes(cfg, num_events) bytes, 16-B aligned, not zeroed, and
 * must pass unchanged from plan to apply.  Its first 8 int64 are the plan's record: [0] n_live, [1] live arena
 * entries (the sum of the walkable run lengths), [2] bad ids, [4] num_events, [5] upto.
 * tgnx_tgn_compact_plan (5 launches) writes only ws: the live bitmap, the exclusive prefix of its popcounts (a
 * fixed-order multi-workgroup integer scan: deterministic) and of the nodes' run lengths, and the record.  An event
 * id outside [0, num_events) in a ring slot or an arena entry, and a run {off, cnt} with cnt < 0 or outside the arena
 * words [0, 2 * num_events), are never used as an index: they are counted into record[2].  Reads buf->nbr / eid /
 * store; buf->ctl must be set (apply writes it).
 * tgnx_tgn_compact_apply (4 launches) gathers src / dst / t / msg of the live rows into the new table (capacity
 * new_capacity rows; msg rows move as 16-byte pieces with a scalar tail), writes kept[new] = old (kept_len slots),
 * remaps buf->eid in place (slots with nbr == -1 untouched), writes the repacked node table and arena into new_store
 * (4 * num_nodes + 2 * new_capacity int64, zero-filled by the caller: node by node, s run then d run; counts
 * unchanged, empty runs at offset 0) and sets ctl BATCH_START = CUR_EID = n_live; no other ctl word changes.  Its
 * kernels check the record first and store nothing when it was made for another row count, counted a bad id, or
 * n_live exceeds new_capacity or kept_len: the caller reads the record after the plan and does not call apply then.
 * Order-preserving renumbering keeps every comparison of event ids (the ring merge ranks by e_id, the stores keep
 * batch order, later rows get ids >= n_live), and the repacked runs fit below 2 * n_live, where the next batch writes.
 * Null or mis-sized arguments: TGNX_EINVAL, nothing launched; num_events >= 2^30: TGNX_ETOOBIG.  One device only.
 * Test: tests/test_gpu_tgn_compact.py. */
size_t tgnx_tgn_compact_ws_bytes(const tgnx_tgn_config* cfg, int64_t num_events);
int tgnx_tgn_compact_plan(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events, int64_t upto,
                          void* ws, size_t ws_bytes, void* stream);
int tgnx_tgn_compact_apply(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events,
                           int64_t new_capacity, int64_t* new_src, int64_t* new_dst, float* new_t, float* new_msg,
                           int64_t* new_store, int64_t* kept, int64_t kept_len, const void* ws, size_t ws_bytes,
                           void* stream);

/* Node-space growth (csrc/tgnx_grow.hip): move what cfg->num_nodes sizes into larger allocations, so
 * that the result is bit for bit the state of an engine built at n_new nodes.  cfg / buf describe the engine as it
 * is (num_nodes = N rows); nothing they point to is written.
 * The new allocations (zero-filled by the caller is fine, not required: every word is written), all NULL-able in old /
 * new pairs so that a loader or a model can grow on its own: */
typedef struct {
  int64_t *nbr, *eid;    /* [row_capacity, ring] */
  float* rt;             /* [row_capacity, ring] */
  int64_t* assoc;        /* [row_capacity] */
  float* memory;         /* [row_capacity, mem_dim] */
  int64_t* last_update;  /* [row_capacity] */
  int32_t* node_gen;     /* [row_capacity] */
  int64_t* store;        /* 4 * n_new + 2 * cfg->num_events int64 */
} tgnx_tgn_grow_out;
/* tgnx_tgn_grow_nodes (2 launches and an 8-byte memset): one kernel walks every row-major tensor — rows [0, N) are
 * copied, rows [N, row_capacity) take what reset_state leaves (nbr / eid -1, rt -1.0f, assoc / memory / last_update /
 * node_gen 0) — in 16-byte pieces where both pointers are 16-B aligned, 4-byte words otherwise; a second re-lays the
 * store: the 4 * N node-table words, zero rows for nodes [N, n_new), then the 2 * cfg->num_events arena words, which
 * move by 4 * (n_new - N) words as a block (run offsets are arena-relative: none is rewritten).  A tensor whose old
 * and new pointer are both NULL is skipped; one of the two alone is TGNX_EINVAL.  row_capacity >= n_new >= N; rows
 * beyond n_new are capacity the caller may hand out later without another call (the store has no such slack: its
 * arena base is 4 * num_nodes words in, so it is re-laid for every new node count, tgnx_tgn_grow_store alone then).
 * *bad (device int64, 8-B aligned; set by the call) counts the store runs {off, cnt} with cnt < 0, or cnt > 0 and
 * not inside the arena words [0, 2 * cfg->num_events): they are counted, never followed — the caller reads it and
 * keeps the old allocations when it is nonzero.  ctl is not touched: TGNX_CTL_GEN does not advance (new rows carry
 * node_gen 0, which no generation equals once a step has run).  The workspace is not moved: its layout depends on
 * num_nodes, the caller allocates tgnx_tgn_ws_bytes of the grown config, zero-filled.
 * NULL cfg / buf / out / bad, n_new < N, row_capacity < n_new: TGNX_EINVAL, nothing launched; 2^31 nodes or more:
 * TGNX_ETOOBIG.  One device only.  Test: tests/test_gpu_tgn_grow.py. */
int tgnx_tgn_grow_nodes(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t n_new, int64_t row_capacity,
                        const tgnx_tgn_grow_out* out, int64_t* bad, void* stream);
int tgnx_tgn_grow_store(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t n_new, int64_t* new_store,
                        int64_t* bad, void* stream);

/* Forgetting nodes (csrc/tgnx_forget.hip): erase a node set F from the stream state in place.  With
 * N = cfg->num_nodes, K = cfg->ring <= 32 and num_events the table's valid rows (cfg->num_events is the capacity):
 *   own rows, v in F    memory[v] = 0, last_update[v] = 0, node_gen[v] = 0, the store's node words {0, 0, 0, 0}, the
 *                       ring row nbr = -1, e_id = -1, t = -1.0f in every slot: what tgnx_tgn_grow_nodes leaves for a
 *                       new row;
 *   ring rows, u not in F   a slot is valid when e_id >= 0 and nbr != -1.  Valid slots whose nbr is in F are removed;
 *                       the surviving (e_id, nbr) pairs keep their order at the front of the row, every other slot
 *                       becomes (-1, -1); the t column becomes ev_t[e_id] of the survivors ranked descending, ties by
 *                       slot (as the ring insert ranks t apart from e_id), -1.0f behind them.  A row that loses
 *                       nothing is not written;
 *   store runs, u not in F  an entry e of the s run is dropped when ev_dst[e] is in F, of the d run when ev_src[e] is;
 *                       the survivors are packed in order at the front of the same run (off unchanged, cnt reduced; an
 *                       emptied run becomes {0, 0}).  Arena words behind a shortened run keep their old values;
 *   nothing else is written (ctl, parameters, the event table: the rows only F kept alive are dead until a compaction).
 * Two calls with one host read between them.  ws is tgnx_tgn_forget_ws_bytes(cfg) bytes, 16-B aligned, not zeroed,
 * and must pass unchanged from plan to apply: [8 int64 record | N-bit bitmap of F | one byte per node].  The record:
 * [0] distinct nodes of F, [1] ring slots to remove, [2] ring rows that lose a slot, [3] store entries to drop (rows
 * and runs of F itself are not counted), [4] bad ids, [5] N, [6] num_events.
 * tgnx_tgn_forget_plan (3 launches; 2 for n = 0) writes only ws.  Duplicate ids are allowed.  Counted into record[4]
 * and never used as an index: an id outside [0, N); a valid ring slot whose nbr is outside [0, N) or whose e_id is
 * >= num_events; a run {off, cnt} with cnt < 0 or outside the arena words [0, 2 * num_events); an arena entry outside
 * [0, num_events) or the other endpoint of its event outside [0, N).  All sums are integer: the record is
 * deterministic.
 * tgnx_tgn_forget_apply (2 launches) rewrites the state as above; both kernels check the record first and store
 * nothing unless it is a clean plan for this N and num_events (the caller reads the record after the plan and does
 * not call apply otherwise).  emb_flags (NULL: none) is plane T of the embedding table's flags: 1 is stored for every
 * v in F and every ring row that is rewritten (idempotent plain stores, as tgnx_embtab_touch).
 * tgnx_ring_forget is the ring part alone, plan and apply in one call (4 launches), for a loader without an engine:
 * with ev_t NULL the t column drops the slots e_id drops (equal to the rule above on a time-ordered stream) and
 * num_events is ignored.  The caller reads the record afterwards: with record[4] != 0 nothing was stored.
 * Null or mis-sized arguments, K > 32: TGNX_EINVAL, nothing launched; 2^31 nodes or more: TGNX_ETOOBIG.  One device
 * only.  Test: tests/test_gpu_tgn_forget.py. */
size_t tgnx_tgn_forget_ws_bytes(const tgnx_tgn_config* cfg);
int tgnx_tgn_forget_plan(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events,
                         const int64_t* ids, int64_t n, void* ws, size_t ws_bytes, void* stream);
int tgnx_tgn_forget_apply(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events, const void* ws,
                          size_t ws_bytes, uint8_t* emb_flags, void* stream);
int tgnx_ring_forget(int64_t* nbr, int64_t* eid, float* rt, const float* ev_t, int64_t num_events, int64_t N,
                     int32_t K, const int64_t* ids, int64_t n, void* ws, size_t ws_bytes, void* stream);

/* train(False): update the memory of every node from its stored messages, clear the stores
 * (memory_module.py:209-215).  Every row is computed from the pre-flush state (:212 updates arange(N) at
 * once).  Graphs with more nodes than the workspace's GRU row capacity run in chunks that read a snapshot
 * of memory / last_update: pass a 16-B aligned device scratch of tgnx_tgn_flush_scratch_bytes(cfg) bytes
 * (0 when one chunk holds every node; scratch may then be NULL). */
size_t tgnx_tgn_flush_scratch_bytes(const tgnx_tgn_config* cfg);
int tgnx_tgn_flush(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, void* scratch, size_t scratch_bytes,
                   void* stream);

/* ---------------------------------------------------------------- per-operator entry points
 * The TGN modules' operators one call each (torch.ops.tgnx.msg_agg_last / msg_agg_mean / gru_update /
 * predictor / edge_attn_fwd / edge_attn_bwd).  The fused steps above do not call these; a caller composing
 * the modules itself does.  Row-major fp32 tensors, int64 indices. */

/* LastAggregator / MeanAggregator (modules/msg_agg.py:15-26).  mode 0 (last): out[r] = msg[argmax_r] with
 * argmax_r the FIRST message (in message order) attaining the largest t among index == r (torch_scatter
 * scatter_max), zeros and argmax_r = n_msg for a row without messages; t is int64 (t_dtype 0, the TGN
 * stores' Long t) or fp32 (t_dtype 1).  mode 1 (mean): out[r] = the messages' sum (sequential, in message
 * order) / their count, zeros for an empty row; t unused (may be NULL).  Deterministic.  An index outside
 * [0, dim_size) is dropped and counted into *n_invalid (a device int64 the caller zeroes; may be NULL).
 * argmax (device int64[dim_size]) may be NULL.  ws: tgnx_msg_agg_ws_bytes(n_msg, dim_size) bytes. */
size_t tgnx_msg_agg_ws_bytes(int64_t n_msg, int64_t dim_size);
int tgnx_msg_agg(int32_t mode, const float* msg, int64_t n_msg, int64_t dim, const int64_t* index, const void* t,
                 int32_t t_dtype, int64_t dim_size, float* out, int64_t* argmax, int64_t* n_invalid, void* ws,
                 size_t ws_bytes, void* stream);

/* TGNMemory.memory_updater (modules/memory_module.py:57,70-78,172): h_out[M,D] = GRUCell (cell 0; weights
 * w_ih [3D,d_in], w_hh [3D,D], torch's r,z,n chunk order) or RNNCell with tanh (cell 1; w_ih [D,d_in],
 * w_hh [D,D]) of x [M,d_in] and h [M,D].  Biases may be NULL.  ws: tgnx_memory_cell_ws_bytes bytes. */
size_t tgnx_memory_cell_ws_bytes(int64_t M, int64_t d_in, int64_t D);
int tgnx_memory_cell(int32_t cell, int64_t M, int64_t d_in, int64_t D, const float* x, const float* h,
                     const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* h_out,
                     void* ws, size_t ws_bytes, void* stream);

/* LinkPredictor (modules/decoder.py:12-27, sigmoid = 1) and EdgePredictor (model_utils.py:165-195,
 * sigmoid = 0: logits): out[i] = w_out · relu(W_src z_src[i mod n_src] + b_src + W_dst z_dst[i] + b_dst) +
 * b_out for i < M (M = n_src: the positive pairs; M = n_src * k: EdgePredictor's `tile` pairing of negative
 * row i with source i mod B, model_utils.py:190).  W_src, W_dst [D,d_in]; w_out [D]; b_out [1]; b_src /
 * b_dst may be NULL.  ws: tgnx_link_predictor_ws_bytes bytes. */
size_t tgnx_link_predictor_ws_bytes(int64_t n_src, int64_t M, int64_t d_in, int64_t D);
int tgnx_link_predictor(int64_t n_src, int64_t M, int64_t d_in, int64_t D, const float* z_src, const float* z_dst,
                        const float* w_src, const float* b_src, const float* w_dst, const float* b_dst,
                        const float* w_out, const float* b_out, int32_t sigmoid, float* out, void* ws,
                        size_t ws_bytes, void* stream);

/* Leave-one-out link logits (csrc/tgnx_explain.hip).  z [n, d_in] and loo_z [n, K, d_in] hold the
 * embedding and the K leave-one-out embeddings of each of n UNIQUE nodes (tgnx_tgn_explain's z and loo_z), count [n]
 * how many of a node's K rows exist; pair p names rows s = src_row[p] and d = dst_row[p].  With logit(a, b) =
 * w_out · relu(W_src a + b_src + W_dst b + b_dst) + b_out (weights as tgnx_link_predictor; b_src / b_dst may be NULL):
 *   base[p] = logit(z[s], z[d]);  src_logit[p, j] = logit(loo_z[s, j], z[d]);  dst_logit[p, j] = logit(z[s], loo_z[d, j])
 * — each side varied alone, also when s == d — and an entry with j >= count of the varied node holds base[p]'s bits.
 * Every unique row is projected once on tgnx_gemm_f32 (4 GEMMs, O(n K D^2) whatever P), then one row kernel runs the
 * 1 + 2 K relu-dot chains of each pair, each a sequential fma chain over the D columns in ascending order: a logit's
 * bits depend on its two rows, not on the grid or the order of the pairs.  A row index outside [0, n) is never
 * dereferenced: the pair's outputs are NaN and *status (device int64, caller-zeroed) becomes 1.  1 <= K <= 64,
 * D <= 256, n, P < 2^24; P = 0 does nothing.  No atomics, no allocation, no host synchronisation.
 * ws: tgnx_link_predictor_loo_ws_bytes bytes.  Test: tests/test_gpu_link_loo.py (float64). */
size_t tgnx_link_predictor_loo_ws_bytes(int64_t n, int64_t K, int64_t P, int64_t d_in, int64_t D);
int tgnx_link_predictor_loo(int64_t n, int64_t K, int64_t P, int64_t d_in, int64_t D, const float* z,
                            const float* loo_z, const int32_t* count, const int64_t* src_row, const int64_t* dst_row,
                            const float* w_src, const float* b_src, const float* w_dst, const float* b_dst,
                            const float* w_out, const float* b_out, float* base /* [P] */,
                            float* src_logit /* [P, K] */, float* dst_logit /* [P, K] */, int64_t* status, void* ws,
                            size_t ws_bytes, void* stream);

/* LinkPredictor over ALL pairs with the selection fused in (csrc/tgnx_topk.hip): for every source row q the k
 * candidates with the largest logit[q][c] = w_out · relu(W_src z_src[q] + b_src + W_dst z_cand[c] + b_dst) + b_out,
 * without a [n_src * n_cand, d_in] operand (the tiled tgnx_link_predictor needs one).  z_src [n_src, d_in], z_cand
 * [n_cand, d_in]; weights as tgnx_link_predictor (b_src / b_dst may be NULL); 1 <= k <= TGNX_TOPK_MAX, D <= 256.
 * The selection is on the LOGIT (fp32 sigmoid is exactly 1.0 above ~17: ties at the top of a trained ranking) under
 * one total order: larger logit first, equal logits by lower candidate position, so the result does not depend on
 * how the work is split; a NaN logit is never selected.  out_idx [n_src, k]: positions into z_cand; out_val
 * [n_src, k]: the selected logits, or their sigmoid when sigmoid = 1.  Slots past n_cand (k > n_cand): idx -1, val
 * -INFINITY (0 with sigmoid = 1).  out_all (optional, [n_src, n_cand]): every logit exactly as the selection
 * compared it (logits, whatever `sigmoid`), written by the same pass.  n_src = 0 does nothing; n_cand = 0 fills the
 * padding.  No float atomics, no allocation, no host synchronisation: graph-capturable and run-to-run identical.
 * ws: tgnx_link_predictor_topk_ws_bytes bytes (Hs, Hd, the per-chunk partial lists; monotone in n_cand). */
#define TGNX_TOPK_MAX 128
size_t tgnx_link_predictor_topk_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k);
int tgnx_link_predictor_topk(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                             const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                             const float* b_dst, const float* w_out, const float* b_out, int32_t k, int32_t sigmoid,
                             float* out_val /* [n_src, k] */, int64_t* out_idx /* [n_src, k] */,
                             float* out_all /* optional [n_src, n_cand], may be NULL */, void* ws, size_t ws_bytes,
                             void* stream);

/* tgnx_link_predictor_topk with per-source exclusions by key.  All four inputs are optional (NULL): cand_key
 * [n_cand] (NULL: a candidate's key is its position); src_key [n_src]: candidate c is excluded for source q when
 * cand_key[c] == src_key[q]; excl_ptr [n_src + 1] and excl_key [nnz]: c is excluded for q when cand_key[c] occurs in
 * excl_key[excl_ptr[q] : excl_ptr[q + 1]] (each segment ascending, duplicates allowed).  Exclusion is by key, so
 * every position holding an excluded key is excluded.  An excluded pair is never selected; with fewer than k
 * candidates left the tail is the padding (idx -1, val -INFINITY, 0 with sigmoid).  out_all gets the UNMASKED logits.
 * Order, ties and NaN as tgnx_link_predictor_topk; a source without exclusions gets exactly its result, and every
 * logit has exactly its bits.  excl_ptr values are clamped into [0, nnz] and a decreasing pair reads as an empty
 * segment; searches stay inside their segment: no content of the arrays causes an access outside their stated sizes
 * (an unsorted segment gives an unspecified selection for that source, nothing worse).  Same workspace, same
 * guarantees (no atomics, no allocation, no host synchronisation). */
size_t tgnx_link_predictor_topk_filtered_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k);
int tgnx_link_predictor_topk_filtered(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                                      const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                                      const float* b_dst, const float* w_out, const float* b_out, int32_t k,
                                      int32_t sigmoid, const int64_t* cand_key /* optional [n_cand] */,
                                      const int64_t* src_key /* optional [n_src] */,
                                      const int64_t* excl_ptr /* optional [n_src + 1] */,
                                      const int64_t* excl_key /* [nnz] */, int64_t nnz,
                                      float* out_val /* [n_src, k] */, int64_t* out_idx /* [n_src, k] */,
                                      float* out_all /* optional [n_src, n_cand] */, void* ws, size_t ws_bytes,
                                      void* stream);

/* The same predictor over a candidate list per source: source q is ranked against the positions
 * list_idx[list_ptr[q] : list_ptr[q + 1]] into z_cand (list_ptr [n_src + 1], list_idx [nnz]; max_len: the host's
 * upper bound on a list's length).  An entry < 0 is skipped silently (how a caller masks an entry); an entry >=
 * n_cand, or at offset >= max_len in its list, is skipped and counted: *n_invalid (optional, device) is incremented.
 * Duplicate entries are separate entries.  out_val [n_src, k]; out_idx [n_src, k] candidate positions; out_slot
 * [n_src, k] the entry's offset inside the source's list; out_logits (optional, [nnz]) every entry's logit, NaN at a
 * skipped entry.  Order: larger logit first, equal logits by lower slot; padding idx / slot -1, val -INFINITY (0 with
 * sigmoid).  Hs and Hd come from the two GEMMs of tgnx_link_predictor_topk and the per-entry logit is its fma chain:
 * for the same inputs the logit of (q, c) has the bits of its out_all[q][c].  list_ptr values are clamped into
 * [0, nnz], a decreasing pair reads as an empty list.  No atomics except the invalid counter, no allocation, no host
 * synchronisation.  ws: tgnx_link_predictor_topk_lists_ws_bytes bytes (monotone in n_cand and max_len). */
size_t tgnx_link_predictor_topk_lists_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k,
                                               int64_t max_len);
int tgnx_link_predictor_topk_lists(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                                   const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                                   const float* b_dst, const float* w_out, const float* b_out, int32_t k,
                                   int32_t sigmoid, const int64_t* list_ptr /* [n_src + 1] */,
                                   const int64_t* list_idx /* [nnz] */, int64_t nnz, int64_t max_len,
                                   float* out_val /* [n_src, k] */, int64_t* out_idx /* [n_src, k] */,
                                   int64_t* out_slot /* [n_src, k] */, float* out_logits /* optional [nnz] */,
                                   int64_t* n_invalid /* optional, device */, void* ws, size_t ws_bytes, void* stream);

/* Where each source's true destination stands among the candidates (csrc/tgnx_topk.hip): the counts
 * a filtered rank needs, without the [n_src, n_cand] logits and without a selection.  z_src, z_cand and the weights
 * as tgnx_link_predictor_topk; only the first n_count <= n_cand rows of z_cand compete (rows past them exist so that
 * a target need not be a competitor); target [n_src]: the position in z_cand of source q's true destination.
 * cand_key, src_key, excl_ptr, excl_key, nnz: optional, with the meaning and the clamping of
 * tgnx_link_predictor_topk_filtered.  With key(c) = cand_key ? cand_key[c] : c, p = target[q] and logit(q, c) the
 * bits of tgnx_link_predictor_topk's out_all[q][c] on the same operands (the same two GEMMs, the same fma chain),
 * the compared set S_q is every c in [0, n_count) with c != p, key(c) != key(p) (the target's node never competes
 * with itself, duplicates included), key(c) != src_key[q], key(c) not in q's exclusion segment, and logit(q, c) not
 * NaN.  The target itself is never removed by the exclusions.  Outputs, each [n_src]: out_tlogit = tl = logit(q, p);
 * out_gt = #{c in S_q: logit > tl}; out_eq = #{c in S_q: logit == tl} (float ==: -0 equals +0); out_n = |S_q|.  The
 * rank under TGB's convention is 1 + gt + eq / 2.  A skipped row (p < 0, p >= n_cand, or tl NaN): gt = eq = 0,
 * tlogit = NaN, n as defined (p out of range: the key(p) rule is vacuous).  n_src = 0 does nothing.  excl_ptr values
 * are clamped into [0, nnz], a decreasing pair reads as an empty segment, a target is read only inside [0, n_cand):
 * no content of the arrays causes an access outside their stated sizes.  Integer atomics only (exact, run-to-run
 * identical), no allocation, no host synchronisation: graph-capturable.  D <= 256.
 * ws: tgnx_link_predictor_rank_ws_bytes bytes (Hs, Hd, the GEMM's; monotone in n_cand). */
size_t tgnx_link_predictor_rank_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D);
int tgnx_link_predictor_rank(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                             const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                             const float* b_dst, const float* w_out, const float* b_out, int64_t n_count,
                             const int64_t* target /* [n_src] */, const int64_t* cand_key /* optional [n_cand] */,
                             const int64_t* src_key /* optional [n_src] */,
                             const int64_t* excl_ptr /* optional [n_src + 1] */,
                             const int64_t* excl_key /* [nnz] */, int64_t nnz, int64_t* out_gt /* [n_src] */,
                             int64_t* out_eq /* [n_src] */, int64_t* out_n /* [n_src] */,
                             float* out_tlogit /* [n_src] */, void* ws, size_t ws_bytes, void* stream);

/* Embedding-space nearest neighbours with the selection fused in (csrc/tgnx_knn.hip): for every query
 * row q the k candidate rows with the largest similarity, without a [n_q, n_cand] score matrix.  z_q [n_q, D] and
 * z_cand [n_cand, D] row-major with pitch D (any alignment), 1 <= D <= 256, 1 <= k <= TGNX_TOPK_MAX.
 * score[q][c] = z_q[q] · z_cand[c] (TGNX_KNN_DOT), or the dot product of the two rows each scaled by 1 / sqrt(Σ z²)
 * (TGNX_KNN_COSINE; a row whose sum of squares is 0 scales by 0: its scores are 0, not NaN).
 * Selection, padding and exclusions as tgnx_link_predictor_topk_filtered: larger score first, equal scores (float ==)
 * by lower candidate position, a NaN score never selected, slots past the candidates left idx -1 / val -INFINITY;
 * cand_key [n_cand], q_key [n_q] (candidate c is out for query q when its key equals q_key[q]: "not myself"),
 * excl_ptr [n_q + 1] / excl_key [nnz] with ascending segments, all optional (NULL); excl_ptr is clamped into
 * [0, nnz], a decreasing pair reads as an empty segment, and no content of the arrays causes an access outside their
 * stated sizes.  out_all (optional, [n_q, n_cand]): the UNMASKED scores exactly as the selection compared them.
 * n_q = 0 does nothing; n_cand = 0 fills the padding.
 * A score is one f32 accumulator's fma chain (v_mfma_f32_16x16x4_f32) from 0 over a fixed permutation of k, the same
 * for every pair (csrc/tgnx_knn.hip states it), and a row norm one fixed order per row: a pair's bits depend on its
 * two rows, D and the metric only, not on n_q, n_cand, the rows' positions or the grid.  No atomics, no allocation,
 * no host synchronisation: graph-capturable, run-to-run identical.
 * ws: tgnx_embed_knn_ws_bytes bytes, 16-byte aligned (the prepared rows, the per-chunk partial lists; monotone in
 * n_cand). */
#define TGNX_KNN_DOT 0
#define TGNX_KNN_COSINE 1
size_t tgnx_embed_knn_ws_bytes(int64_t n_q, int64_t n_cand, int64_t D, int32_t k);
int tgnx_embed_knn(int64_t n_q, int64_t n_cand, int64_t D, const float* z_q, const float* z_cand, int32_t metric,
                   int32_t k, const int64_t* cand_key /* optional [n_cand] */, const int64_t* q_key /* optional [n_q] */,
                   const int64_t* excl_ptr /* optional [n_q + 1] */, const int64_t* excl_key /* [nnz] */, int64_t nnz,
                   float* out_val /* [n_q, k] */, int64_t* out_idx /* [n_q, k] */,
                   float* out_all /* optional [n_q, n_cand] */, void* ws, size_t ws_bytes, void* stream);

/* TransformerConv's attention (modules/emb_module.py:21-29; PyG TransformerConv, concat, no beta): for
 * destination i with incoming edges p in [indptr[i], indptr[i+1]) (rows of the per-edge k, v, e [E, H*C];
 * q [n_dst, H*C]), per head h: a_p = q_i·(k_p + e_p) / sqrt(C), α = softmax over i's edges (max subtracted,
 * + 1e-16 in the denominator), out_i = Σ_p α_p (v_p + e_p) (the root weight / skip is the caller's Linear).
 * e may be NULL (no edge features).  alpha [E, H] is written.  1 <= heads <= 8, heads * C <= 256.  indptr is
 * clamped to [0, n_edges].  No attention dropout (eval, or dropout 0; tgnx_edge_attn_drop_fwd below has it).
 * Backward: dq [n_dst, H*C], dk / dv / de [E, H*C] (de = dk + dv, needed only with e) from dout and alpha.
 * indptr need not span all n_edges rows.  An edge row that no destination owns (a row before indptr[0] or from
 * indptr[n_dst] on, indptr non-decreasing; every row when n_dst == 0) takes part in nothing: both calls write
 * every row of their per-edge outputs, and such a row gets alpha = 0 and dk = dv = de = 0. */
int tgnx_edge_attn_fwd(int64_t n_dst, int64_t n_edges, int32_t heads, int32_t channels, const float* q,
                       const float* k, const float* v, const float* e, const int64_t* indptr, float* out,
                       float* alpha, void* stream);
int tgnx_edge_attn_bwd(int64_t n_dst, int64_t n_edges, int32_t heads, int32_t channels, const float* dout,
                       const float* q, const float* k, const float* v, const float* e, const int64_t* indptr,
                       const float* alpha, float* dq, float* dk, float* dv, float* de, void* stream);

/* The same attention with attention dropout, in PyG's order (softmax, then dropout on α):
 *   out_i = Σ_p (α_p m_p)(v_p + e_p),   m[p,h] = keep32(drop_base(seed, stream_id, dkey_i, ekey_p), h, p, inv)
 *   dkey_i = dst_key ? dst_key[i] : i,  ekey_p = edge_key ? edge_key[p] : p  (full 64-bit keys),  inv = 1 / (1 - p)
 * drop_base / keep32 are the counter-based hash of csrc/tgnx_math.h (m is 0 or inv).  alpha [E, H] receives the
 * softmax BEFORE dropout (PyG's _alpha); the backward takes that alpha and recomputes the mask from (p, seed,
 * stream_id, keys), so no mask is stored:
 *   dα_p = m_p (dout_i·(v_p + e_p)),  g_p = α_p (dα_p − Σ α dα) / sqrt(C),  dq_i = Σ g_p (k_p + e_p),
 *   dk_p = g_p q_i,  dv_p = α_p m_p dout_i,  de_p = dk_p + dv_p.
 * A (destination, head) that loses every edge gives a zero head block in out and contributes zeros; nothing is
 * divided by a kept count.  p must be finite with 0 <= p < 1 (TGNX_EINVAL before any launch otherwise); p = 0 gives
 * the bits of tgnx_edge_attn_fwd / _bwd.  dst_key [n_dst] and edge_key [n_edges] are optional (NULL: the row
 * numbers).  Sizes, indptr clamping and the rows no destination owns are as for the pair above.  No atomics, no
 * workspace, no host synchronisation: graph-capturable, run-to-run identical.
 * With stream_id = 7 (the engine's conv; 9 for conv2), dst_key = the centres' node ids, edge_key = the edges' event
 * ids and seed = a batch's ctl[TGNX_CTL_SEED], the mask is the one tgnx_tgn_train_step draws for that batch. */
int tgnx_edge_attn_drop_fwd(int64_t n_dst, int64_t n_edges, int32_t heads, int32_t channels, const float* q,
                            const float* k, const float* v, const float* e, const int64_t* indptr, float* out,
                            float* alpha, float p, uint64_t seed, uint64_t stream_id,
                            const int64_t* dst_key /* optional [n_dst] */,
                            const int64_t* edge_key /* optional [n_edges] */, void* stream);
int tgnx_edge_attn_drop_bwd(int64_t n_dst, int64_t n_edges, int32_t heads, int32_t channels, const float* dout,
                            const float* q, const float* k, const float* v, const float* e, const int64_t* indptr,
                            const float* alpha, float* dq, float* dk, float* dv, float* de, float p, uint64_t seed,
                            uint64_t stream_id, const int64_t* dst_key /* optional [n_dst] */,
                            const int64_t* edge_key /* optional [n_edges] */, void* stream);

/* ---------------------------------------------------------------- per-operator backward (csrc/tgnx_ops_bwd.hip)
 * What torch autograd needs to train a composition of the operators above (tgnx/ops.py, tgnx/nn.py).  Same
 * conventions: row-major fp32, int64 indices, caller-provided workspace, no allocation.  Every one of them is
 * run-to-run deterministic: no float atomics, column and row sums in an order fixed by the shapes.  Contractions
 * run on tgnx_gemm_f32. */

/* out[c] = Σ_m x[m*ldx + c] for c < N (the bias gradients), ldx >= N.  Order: rows in chunks of 256, within a
 * chunk four strided sequential partial sums added in order, then the chunks in order.  M = 0 gives zeros.
 * ws: tgnx_col_sum_ws_bytes(M, N) bytes. */
size_t tgnx_col_sum_ws_bytes(int64_t M, int64_t N);
int tgnx_col_sum(int64_t M, int64_t N, const float* x, int64_t ldx, float* out, void* ws, size_t ws_bytes,
                 void* stream);

/* Backward of tgnx_memory_cell given dh_out [M,D]: the pre-activations are recomputed (two GEMMs), one elementwise
 * kernel forms the gate gradients (GRU in torch's r,z,n order; RNN: dh_out (1 − h'²)), then dx [M,d_in] = dgi W_ih,
 * dh [M,D] = dh_out z + dgh W_hh, dw_ih = dgi^T x, dw_hh = dgh^T h (shapes of w_ih / w_hh) and the bias gradients
 * [3D] (GRU) / [D] (RNN) by column sums.  Any output pointer may be NULL to skip it; b_ih / b_hh may be NULL as in
 * the forward.  ws: tgnx_memory_cell_bwd_ws_bytes bytes. */
size_t tgnx_memory_cell_bwd_ws_bytes(int64_t M, int64_t d_in, int64_t D);
int tgnx_memory_cell_bwd(int32_t cell, int64_t M, int64_t d_in, int64_t D, const float* dh_out, const float* x,
                         const float* h, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                         float* dx, float* dh, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* ws,
                         size_t ws_bytes, void* stream);

/* Backward of tgnx_link_predictor given dout [M] (the gradient of the sigmoid output when sigmoid = 1, of the
 * logits otherwise).  With g_i = dout_i (σ(1 − σ) of the recomputed output) and da[i] = g_i w_out [pre-activation
 * > 0]: dz_dst [M,d_in] = da W_dst; dz_src [n_src,d_in] = dhs W_src with dhs[j] = Σ_{i ≡ j (mod n_src)} da[i] in
 * increasing i (the `tile` pairing); dw_src / dw_dst [D,d_in], db_src / db_dst [D], dw_out [D], db_out [1].  Any
 * output pointer may be NULL.  ws: tgnx_link_predictor_bwd_ws_bytes bytes. */
size_t tgnx_link_predictor_bwd_ws_bytes(int64_t n_src, int64_t M, int64_t d_in, int64_t D);
int tgnx_link_predictor_bwd(int64_t n_src, int64_t M, int64_t d_in, int64_t D, const float* dout, const float* z_src,
                            const float* z_dst, const float* w_src, const float* b_src, const float* w_dst,
                            const float* b_dst, const float* w_out, const float* b_out, int32_t sigmoid,
                            float* dz_src, float* dz_dst, float* dw_src, float* db_src, float* dw_dst, float* db_dst,
                            float* dw_out, float* db_out, void* ws, size_t ws_bytes, void* stream);

/* TimeEncoder ([ext] torch_geometric TimeEncoder; modules/time_enc.py is absent from the reference):
 * out[n,D] = cos(fmaf(w[c], t[i], b[c])) with the exact argument reduction of the fused steps (csrc/tgnx_math.h).
 * Backward: dw[c] = Σ_i −sin(·) t[i] dout[i,c], db[c] = Σ_i −sin(·) dout[i,c], fused as one column reduction (no
 * [n,D] temporary); dw / db may be NULL.  t is data: no gradient.  ws: tgnx_time_encode_bwd_ws_bytes bytes. */
int tgnx_time_encode(int64_t n, int64_t D, const float* t, const float* w, const float* b, float* out, void* stream);
size_t tgnx_time_encode_bwd_ws_bytes(int64_t n, int64_t D);
int tgnx_time_encode_bwd(int64_t n, int64_t D, const float* t, const float* w, const float* b, const float* dout,
                         float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* TimeEmbedding (JODIE's projection, modules/emb_module.py:32-52): out[n,D] = x (1 + w[c] rel_t[i] + b[c]).
 * Backward: dx = dout (1 + w rel_t + b), dw[c] = Σ_i dout x rel_t, db[c] = Σ_i dout x; dx / dw / db may be NULL.
 * ws: tgnx_time_embedding_bwd_ws_bytes bytes. */
int tgnx_time_embedding(int64_t n, int64_t D, const float* x, const float* rel_t, const float* w, const float* b,
                        float* out, void* stream);
size_t tgnx_time_embedding_bwd_ws_bytes(int64_t n, int64_t D);
int tgnx_time_embedding_bwd(int64_t n, int64_t D, const float* x, const float* rel_t, const float* w, const float* b,
                            const float* dout, float* dx, float* dw, float* db, void* ws, size_t ws_bytes,
                            void* stream);

/* Backward of tgnx_msg_agg.  last: dmsg [n_msg,dim] is zeroed, then dmsg[argmax[r]] = dout[r] for the rows with
 * argmax[r] < n_msg (argmax as the forward wrote it): a scatter, exact.  mean: dmsg[p] = dout[index[p]] /
 * count[index[p]], the counts from an integer histogram; an index outside [0, dim_size) gets a zero row and is
 * counted into *n_invalid (a device int64 the caller zeroes; may be NULL).  ws (mean):
 * tgnx_msg_agg_mean_bwd_ws_bytes(dim_size) bytes. */
int tgnx_msg_agg_last_bwd(const float* dout, const int64_t* argmax, int64_t dim_size, int64_t dim, int64_t n_msg,
                          float* dmsg, void* stream);
size_t tgnx_msg_agg_mean_bwd_ws_bytes(int64_t dim_size);
int tgnx_msg_agg_mean_bwd(const float* dout, const int64_t* index, int64_t n_msg, int64_t dim, int64_t dim_size,
                          float* dmsg, int64_t* n_invalid, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- device message store (csrc/tgnx_memstore.hip)
 * The stores of TGNMemory / DyRepMemory (modules/memory_module.py:140-145, :180-207; DyRep :376-412) behind
 * tgnx.nn.TGNMemory.  Times here are int64 (PyG's convention: TGNMemory keeps t and last_update as Long).
 *   event log   src, dst, t int64[cap], raw_msg fp32[cap, msg_dim]: append-only, every batch once
 *   node table  int64[4 N] {s_off, s_cnt, d_off, d_cnt} per node (16-B aligned; all zero = every store empty)
 *   arena       int64[2 cap] of log slots: the batch that starts at log slot s owns entries [2s, 2s + 2B), its slots
 *               sorted stably by src, then sorted stably by dst (a node's stored events keep batch order)
 * The fill level lives on the host (every put's B is known there); resetting = zeroing the node table and starting
 * again at slot 0.  Dead log entries are not compacted.  Deterministic: no float atomics. */

/* _update_msg_store of both directions (memory_module.py:133-134, :180-191), one launch: appends the batch at log
 * slots [start, start + B), fills its arena entries and points every distinct src (dst) at its new run in the s (d)
 * store.  sorted / perm int64[2 B]: the batch's src ids sorted stably and the permutation that sorts them
 * (indices in [0, B)), then the same for dst (torch.sort(stack([src, dst]), dim=1, stable=True)).  A node id outside
 * [0, num_nodes) gets no run, a perm entry outside [0, B) is replaced by 0; both are counted into *n_bad (device
 * int64, accumulated; may be NULL). */
int tgnx_memstore_put(const int64_t* src, const int64_t* dst, const int64_t* t, const float* raw_msg, int64_t B,
                      int64_t msg_dim, const int64_t* sorted, const int64_t* perm, int64_t start, int64_t cap,
                      int64_t num_nodes, int64_t* log_src, int64_t* log_dst, int64_t* log_t, float* log_raw,
                      int64_t* arena, int64_t* node_tab, int64_t* n_bad, void* stream);

/* The stored events of a node set n_id[M] (no duplicates), in the order [s store of n_id[0], n_id[1], ...; d store of
 * n_id[0], ...] (_compute_msg twice + the cat of memory_module.py:156-168), in two calls around the one size the host
 * must know.  Both use one workspace of tgnx_memstore_gather_ws_bytes(M) bytes, which carries the scanned tile
 * offsets from the first call to the second.
 * count: totals (device int64[3]) = {n_s, n_d, invalid ids}: the messages of either direction and the entries of n_id
 *   outside [0, num_nodes) plus *put_bad (the puts' count; may be NULL).  Counts are scanned on the device.
 * gather: for message p < n_s + n_d: out_slot[p] its log slot (-1: a corrupt table entry), out_owner[p] the position
 *   of its owner in n_id (the reference's _assoc[idx]), out_t[p] its time; out_lu[i] for i < M the max of t over node
 *   n_id[i]'s messages of both directions, 0 without any (scatter(t, idx, reduce="max")[n_id], :176).  n_s / n_d as
 *   count returned them; fill = log slots in use. */
size_t tgnx_memstore_gather_ws_bytes(int64_t M);
int tgnx_memstore_count(const int64_t* node_tab, int64_t num_nodes, const int64_t* n_id, int64_t M,
                        const int64_t* put_bad, int64_t* totals, void* ws, size_t ws_bytes, void* stream);
int tgnx_memstore_gather(const int64_t* node_tab, int64_t num_nodes, const int64_t* arena, const int64_t* log_t,
                         int64_t fill, const int64_t* n_id, int64_t M, int64_t n_s, int64_t n_d, int64_t* out_slot,
                         int64_t* out_owner, int64_t* out_t, int64_t* out_lu, const void* ws, size_t ws_bytes,
                         void* stream);

/* The message inputs of _compute_msg (memory_module.py:193-207) for the gathered slots, one wave per row:
 * out[p] = [memory[src] | memory[dst] | raw_msg | cos(fmaf(w, t_rel, b))], width 2 mem_dim + msg_dim + time_dim, with
 * (src, dst) = the stored event's (src, dst) for p < n_s and (dst, src) for the d store's rows, t_rel[p] = (fp32)
 * (t - last_update[src]) taken in int64 (also written out: what tgnx_time_encode_bwd needs), the cosine with the exact
 * argument reduction of tgnx_time_encode.  A column group moves as 16-B vectors when its offsets and widths allow and
 * element by element otherwise.  DyRepMemory (:387-408): with emb [emb_rows, mem_dim] and emb_flags bit 0 (bit 1) an
 * src (dst) endpoint x that is in n_id[M] takes emb[assoc[x]] instead of its memory row; x is in n_id iff
 * stamp[x] < M and n_id[stamp[x]] == x, stamp being the node -> position map the gather's caller wrote for n_id
 * (TGNMemory._assoc; stale entries of earlier node sets fail the second test).  emb NULL: emb_flags is ignored. */
int tgnx_memstore_build_msg(const int64_t* slot, int64_t n_msg, int64_t n_s, const int64_t* log_src,
                            const int64_t* log_dst, const int64_t* log_t, const float* log_raw, int64_t fill,
                            int64_t num_nodes, int64_t mem_dim, int64_t msg_dim, int64_t time_dim, const float* memory,
                            const int64_t* last_update, const float* w, const float* b, const float* emb,
                            int64_t emb_rows, const int64_t* assoc, const int64_t* stamp, const int64_t* n_id, int64_t M,
                            int32_t emb_flags, float* out, float* t_rel, void* stream);

/* ---------------------------------------------------------------- node property prediction (csrc/tgnx_nodeprop.hip)
 * NodePredictor (modules/decoder.py:30-41), its soft-target cross-entropy and NDCG@k (TGB's tgbn-* task).  Row-major
 * fp32, caller-provided workspace, no allocation, no float atomics: every result is run-to-run bit-identical and
 * independent of the grid. */
#define TGNX_NODE_MAX_D 128
#define TGNX_NODE_MAX_C 4096
#define TGNX_NODE_MAX_K 128

/* logits [M,C] = W2 relu(W1 z + b1) + b2 for z [M,D], w1 [D,D], w2 [C,D] (torch Linear layout), b1 [D] / b2 [C]
 * (either may be NULL).  Two launches of the f32 MFMA GEMM core, bias and ReLU in their epilogues.  h [M,D] (the
 * hidden rows relu(W1 z + b1), what the backward needs) is written when non-NULL; otherwise the hidden rows stay in
 * the workspace.  1 <= D <= TGNX_NODE_MAX_D, 1 <= C <= TGNX_NODE_MAX_C, 0 <= M < 2^24. */
size_t tgnx_node_predictor_ws_bytes(int64_t M, int64_t D, int64_t C);
int tgnx_node_predictor(int64_t M, int64_t D, int64_t C, const float* z, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* logits, float* h, void* ws, size_t ws_bytes,
                        void* stream);

/* Backward given dlogits [M,C] and the saved z, h: dw2 [C,D] = dlogits^T h, db2 [C], dh = (dlogits W2) (h > 0) (the
 * mask in the GEMM's epilogue), dw1 [D,D] = dh^T z, db1 [D], dz [M,D] = dh W1.  Any output pointer may be NULL.
 * M = 0 zeroes the parameter gradients.  ws: tgnx_node_predictor_bwd_ws_bytes bytes. */
size_t tgnx_node_predictor_bwd_ws_bytes(int64_t M, int64_t D, int64_t C);
int tgnx_node_predictor_bwd(int64_t M, int64_t D, int64_t C, const float* dlogits, const float* z, const float* h,
                            const float* w1, const float* w2, float* dz, float* dw1, float* db1, float* dw2,
                            float* db2, void* ws, size_t ws_bytes, void* stream);

/* One pass over each row of logits [M,C] against dense targets y [M,C] (>= 0, any row sum), a wave per row:
 *   loss_rows[i] = lse_i Σ_c y_ic − Σ_c y_ic l_ic                      (soft-target cross-entropy of the row)
 *   dlogits[i,c] = (softmax(l_i)_c Σ_c' y_ic' − y_ic) scale            (scale = 1 / M for the mean loss)
 *   ndcg[i]      = sklearn's ndcg_score(y_i, l_i, k) with tie averaging, float64: with gt_c / eq_c the classes
 *                  scoring above / equal to c (c included), DCG = Σ_{c: y_c > 0} y_c (cum[min(gt_c + eq_c, k)] −
 *                  cum[min(gt_c, k)]) / eq_c, IDCG the same with y ranked by itself, 0 where IDCG = 0.
 * cum: k + 1 doubles on the device, cum[j] = Σ_{r=1..j} 1 / log2(r + 1) computed by the host.  Each of loss_rows,
 * loss_mean (one float: scale Σ_i loss_rows[i] in a fixed order, a second one-workgroup launch; needs loss_rows),
 * dlogits and ndcg may be NULL.  Row sums run lane-strided over the 64-class chunks in order, then across the wave;
 * DCG / IDCG add their float64 terms in class order.  1 <= C <= TGNX_NODE_MAX_C, 1 <= k <= TGNX_NODE_MAX_K.  Rows
 * whose logits are all -inf or hold a NaN are outside the domain. */
int tgnx_node_loss_ndcg(int64_t M, int64_t C, int32_t k, const float* logits, const float* y, const double* cum,
                        float scale, float* loss_rows, float* loss_mean, float* dlogits, double* ndcg, void* stream);

/* ---------------------------------------------------------------- test hooks
 * The GEMM core (csrc/tgnx_gemm.h) on each tile config the library compiles, for tests/test_gpu_gemm_core.py; no
 * product path calls these.  cfg picks the config through the alias the step itself uses (so a build-variant
 * macro changes the probe as well). */
enum {
  TGNX_GEMM_PROBE_G32 = 0,  /* 16x16 wave split-K tiles, direct operands, 2 slabs per load round */
  TGNX_GEMM_PROBE_G32L = 1, /* the same, 3 slabs per round (also the dX_enc GEMM's default) */
  TGNX_GEMM_PROBE_GW = 2,   /* 32x32, 2x2 wave grid, register-layout split-K partials */
  TGNX_GEMM_PROBE_G64 = 3,  /* 64x64 */
  TGNX_GEMM_PROBE_GD = 4    /* the small-shape config of the dense fp32 GEMM entry above */
};
/* C[M,N] = op(A) op(B) (+ bias) (+ C if accumulate), operands as in the dense fp32 GEMM entry above.
 * smax = 0: a direct GEMM; smax > 0: deferred split-K over at most smax splits, then the fixup launch.
 * grid_cap > 0 caps the grid (rounded up to a multiple of 8): workgroups loop over the tiles past it.
 * M, N, K are the capacity shape; dims_dev is NULL or three int32 on the device {Mr, Nr, Kr}, the runtime sizes
 * (each at most its capacity; an entry < 0 means that size is not passed to the kernel).  The call reads
 * dims_dev back (it synchronises the stream) to see which entries are passed.  Every buffer must cover the
 * capacity shape.  a_rows (NULL or M int64 on the device, needs trans_a = 0): row m of op(A) is row a_rows[m] of
 * A, through a two-phase gather loader; the caller keeps every entry within A's rows.
 * ws holds the bytes the _ws_bytes call returns for (cfg, smax, M, N, K). */
size_t tgnx_gemm_probe_ws_bytes(int32_t cfg, int32_t smax, int64_t M, int64_t N, int64_t K);
int tgnx_gemm_probe(int32_t cfg, int32_t smax, int32_t grid_cap, int64_t M, int64_t N, int64_t K,
                    const int32_t* dims_dev, const float* A, int64_t lda, int32_t trans_a, const int64_t* a_rows,
                    const float* B, int64_t ldb, int32_t trans_b, float* C, int64_t ldc, const float* bias,
                    int32_t accumulate, void* ws, size_t ws_bytes, void* stream);
/* Several jobs in one GEMM launch and one fixup launch.  jobs[3]: jobs[0] a direct G32 GEMM, C = A B^T (smax
 * unused); jobs[1] a deferred GW GEMM, C = A^T B; jobs[2] a deferred GW GEMM, C = A B^T (A, B row-major as stored:
 * A is M x K, or K x M for A^T; B is N x K, or K x N for jobs[1]); each with its bias / accumulate epilogue.  The
 * GEMM launch also hosts nb plain blocks, block b adding 1 to marks[b].  The fixup launch sums jobs[1] and jobs[2]
 * and hosts tail_blocks extra blocks, the first `head` of them at the front of the grid (0 <= head <= tail_blocks),
 * extra block b adding 1 to tail_marks[b].  fix_blocks (may be NULL): one int32 per output tile of jobs[1], then of
 * jobs[2] (row-major tile order, 32x32 tiles unless the build changes GW): the block of the fixup grid that finished
 * that tile. */
typedef struct tgnx_gemm_probe_job {
  int64_t M, N, K;
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  float* C;
  int64_t ldc;
  const float* bias;
  int32_t accumulate, smax;
} tgnx_gemm_probe_job;
size_t tgnx_gemm_probe_batch_ws_bytes(const tgnx_gemm_probe_job* jobs);
int tgnx_gemm_probe_batch(const tgnx_gemm_probe_job* jobs, int32_t nb, int32_t* marks, int32_t head,
                          int32_t tail_blocks, int32_t* tail_marks, int32_t* fix_blocks, void* ws, size_t ws_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGNX_H */
