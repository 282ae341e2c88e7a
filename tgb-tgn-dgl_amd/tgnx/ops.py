"""torch.ops.tgnx — libtgnx's C ABI registered as PyTorch operators (csrc/tgnx_torch.cpp).

    from tgnx import ops; ops.load()
    n_id, edge_index, e_id, t = torch.ops.tgnx.ring_sample(nbr, e_id, t, assoc, n_id)

Ops: ring_reset / ring_sample / ring_insert (LastNeighborLoader, neighbor_loader.py:26-109), neg_sample
(NegLinkSamplerDest, neg_sampler.py:8-23), block_ids (dependencyGraph.py:8-49, host tensors), tcsr_build /
tcsr_sample (TGL t-CSR, utils.py:73), gemm_f32 (MFMA fp32 GEMM), and the TGN modules' operators one call each
(csrc/tgnx_ops.hip): msg_agg_last / msg_agg_mean (LastAggregator / MeanAggregator, modules/msg_agg.py:15-26),
gru_update (TGNMemory's GRUCell / RNNCell, memory_module.py:70-78), predictor (LinkPredictor decoder.py:12-27;
EdgePredictor model_utils.py:165-195), predictor_topk (LinkPredictor over all pairs with the top-k selection fused
in, csrc/tgnx_topk.hip; `link_topk` below; predictor_topk_filtered / predictor_topk_lists: the same with per-source
exclusions by key / a candidate list per source; predictor_loo: the logit of explicit pairs with one side's embedding
replaced by each of its leave-one-out rows, csrc/tgnx_explain.hip; `link_loo` below), embed_knn (nearest neighbours in embedding space, dot or cosine, on the
f32 MFMA with the same selection and exclusions, csrc/tgnx_knn.hip; `embed_knn` below) and edge_attn_fwd / edge_attn_bwd (TransformerConv's attention,
emb_module.py:21-29; `edge_attention` below wraps the pair as an autograd function; edge_attn_drop_fwd /
edge_attn_drop_bwd: the same with attention dropout under the engine's counter-based mask), time_encode (TimeEncoder)
and time_embedding (TimeEmbedding, emb_module.py:32-52).  The backward halves (csrc/tgnx_ops_bwd.hip: col_sum,
gru_update_bwd, predictor_bwd, time_encode_bwd, time_embedding_bwd, msg_agg_last_bwd, msg_agg_mean_bwd) sit
behind the autograd functions below — memory_cell, link_predictor, time_encode, time_embedding, aggregate_last,
aggregate_mean, linear — which tgnx/nn.py's modules call.  memstore_put / memstore_count / memstore_gather /
memstore_build_msg (csrc/tgnx_memstore.hip) are the device message store of tgnx.nn.TGNMemory / DyRepMemory
(memory_module.py:140-145, :180-207); `build_messages` below is memstore_build_msg with the time encoder's
gradient.  node_predictor / node_predictor_bwd / node_loss_ndcg (csrc/tgnx_nodeprop.hip) are TGB's node property
prediction: NodePredictor (decoder.py:30-41) and the row kernel giving soft-target cross-entropy, its gradient and
NDCG@k in one pass; `node_predictor`, `soft_cross_entropy`, `ndcg_at_k`, `node_loss_ndcg` below.  No CPU fallback:
loading needs the built library (make -C tgb-tgn-dgl_amd) and the device ops need a HIP device.
"""
from __future__ import annotations

import os

import torch

OPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtgnx_torch.so")
OPS = ("ring_reset", "ring_sample", "ring_insert", "neg_sample", "block_ids", "tcsr_build", "tcsr_sample", "gemm_f32",
       "msg_agg_last", "msg_agg_mean", "gru_update", "predictor", "predictor_topk", "edge_attn_fwd", "edge_attn_bwd",
       "edge_attn_drop_fwd", "edge_attn_drop_bwd",
       "predictor_topk_filtered", "predictor_topk_lists", "predictor_rank", "predictor_loo", "embed_knn",
       "sample_recent", "insert_recent", "reset",
       "col_sum", "gru_update_bwd", "predictor_bwd", "time_encode", "time_encode_bwd", "time_embedding",
       "time_embedding_bwd", "msg_agg_last_bwd", "msg_agg_mean_bwd",
       "memstore_put", "memstore_count", "memstore_gather", "memstore_build_msg",
       "pair_index_build", "pair_index_contains", "negs_hist_rnd",
       "pairset_insert", "pairset_lookup", "pairset_select",
       "node_predictor", "node_predictor_bwd", "node_loss_ndcg")
_loaded = False


def load():
    """Register torch.ops.tgnx.* (idempotent); returns the op namespace."""
    global _loaded
    if not _loaded:
        if not os.path.exists(OPS_PATH):
            raise RuntimeError(f"tgnx: {OPS_PATH} is missing — build it with `make -C tgb-tgn-dgl_amd`")
        torch.ops.load_library(OPS_PATH)
        _loaded = True
    return torch.ops.tgnx


class _EdgeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, e, indptr, heads):
        out, alpha = load().edge_attn_fwd(q, k, v, e, indptr, heads)
        ctx.save_for_backward(q, k, v, e if e is not None else q.new_empty(0), indptr, alpha)
        ctx.heads, ctx.has_e = heads, e is not None
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, dout, _dalpha):
        q, k, v, e, indptr, alpha = ctx.saved_tensors
        dq, dk, dv, de = load().edge_attn_bwd(dout.contiguous(), q, k, v, e if ctx.has_e else None, indptr, alpha,
                                              ctx.heads)
        return dq, dk, dv, (de if ctx.has_e else None), None, None


class _EdgeAttentionDrop(torch.autograd.Function):
    """edge_attn_drop_fwd / _bwd: α (before dropout) and the keys are saved, the mask is not — the backward
    recomputes it from (p, seed, stream, keys)."""

    @staticmethod
    def forward(ctx, q, k, v, e, indptr, heads, p, seed, stream, dst_key, edge_key):
        out, alpha = load().edge_attn_drop_fwd(q, k, v, e, indptr, heads, p, seed, stream, dst_key, edge_key)
        empty = indptr.new_empty(0)
        ctx.save_for_backward(q, k, v, e if e is not None else q.new_empty(0), indptr, alpha,
                              dst_key if dst_key is not None else empty, edge_key if edge_key is not None else empty)
        ctx.heads, ctx.has_e, ctx.drop = heads, e is not None, (p, seed, stream)
        ctx.has_keys = (dst_key is not None, edge_key is not None)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, dout, _dalpha):
        q, k, v, e, indptr, alpha, dst_key, edge_key = ctx.saved_tensors
        p, seed, stream = ctx.drop
        dq, dk, dv, de = load().edge_attn_drop_bwd(
            dout.contiguous(), q, k, v, e if ctx.has_e else None, indptr, alpha, ctx.heads, p, seed, stream,
            dst_key if ctx.has_keys[0] else None, edge_key if ctx.has_keys[1] else None)
        return (dq, dk, dv, (de if ctx.has_e else None)) + (None,) * 7


ATTN_DROPOUT_STREAM = 7  # the hash stream of the engine's conv attention dropout (9: conv2)


def step_seed(base_seed: int, nb: int) -> int:
    """The engine's per-batch dropout seed, mix64(base_seed ^ mix64(nb)) >> 1 (splitmix64's output function, nb =
    the batch counter after its advance), in host integer arithmetic."""
    m = (1 << 64) - 1

    def mix64(z):
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    return mix64((int(base_seed) & m) ^ mix64(int(nb) & m)) >> 1


def edge_attention(q, k, v, e, indptr, heads, dropout=0.0, seed=None, stream=ATTN_DROPOUT_STREAM, dst_key=None,
                   edge_key=None):
    """TransformerConv's attention (PyG semantics, emb_module.py:21-29) with autograd: q [n_dst, H*C] per
    destination; k, v, e [E, H*C] per edge, destination i's edges the rows [indptr[i], indptr[i+1]) (e may be
    None).  Returns (out [n_dst, H*C], alpha [E, H]); gradients flow to q, k, v, e.  1 <= heads <= 8 and
    H*C <= 256 (RuntimeError otherwise).  indptr (non-decreasing) need not span all E rows: an edge row that no
    destination owns, before indptr[0] or from indptr[-1] on, and every row when n_dst == 0, has alpha = 0 and
    receives zero gradients in k, v and e.

    dropout > 0 applies attention dropout after the softmax (PyG's order): out_i = Σ_p (α_p m_p)(v_p + e_p) with the
    counter-based mask m[p, h] = keep32(drop_base(seed, stream, dst_key[i], edge_key[p]), h) of csrc/tgnx_math.h
    (tests/dropout_ref.py restates it), 0 or 1 / (1 - dropout); alpha stays the softmax before dropout.  seed (an int in
    [0, 2^63)) is required then (ValueError without); dst_key [n_dst] / edge_key [E] are optional int64 tensors
    (default: the row numbers).  With stream 7, the centres' node ids, the edges' event ids and a batch's step seed
    the mask is the fused train step's.  dropout == 0 is exactly the call without these arguments."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    e = None if e is None else e.contiguous()
    if dropout == 0:
        return _EdgeAttention.apply(q, k, v, e, indptr, int(heads))
    if seed is None:
        raise ValueError("edge_attention: dropout > 0 needs a seed (the mask is a function of it, not of torch's RNG)")
    seed = int(seed)
    if not 0 <= seed < (1 << 63):
        raise ValueError("edge_attention: seed must be a non-negative integer below 2^63")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("edge_attention: dropout must be in [0, 1)")
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    return _EdgeAttentionDrop.apply(q, k, v, e, indptr, int(heads), float(dropout), seed, int(stream), c(dst_key),
                                    c(edge_key))


def _grads(outs, need):
    """The backward ops return an empty tensor for a gradient that was not asked for: None to autograd."""
    return tuple(g if n else None for g, n in zip(outs, need))


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return load().gemm_f32(x, weight, bias, False, True)

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        ns, dout = load(), dout.contiguous()
        nx, nw, nb = ctx.needs_input_grad
        dx = ns.gemm_f32(dout, weight, None, False, False) if nx else None
        dw = None
        if nw:  # dW = dout^T x (a contraction over the rows: zero without rows)
            dw = ns.gemm_f32(dout, x, None, True, False) if x.size(0) else torch.zeros_like(weight)
        db = ns.col_sum(dout) if nb and ctx.has_bias else None
        return dx, dw, db


def linear(x, weight, bias=None):
    """torch.nn.functional.linear on the MFMA GEMM: x [M, in] weight^T [out, in] + bias; dx and dW by gemm_f32,
    db by col_sum."""
    return _Linear.apply(x.contiguous(), weight.contiguous(), None if bias is None else bias.contiguous())


class _MemoryCell(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, w_ih, w_hh, b_ih, b_hh, cell):
        ctx.save_for_backward(x, h, w_ih, w_hh, *(b for b in (b_ih, b_hh) if b is not None))
        ctx.cell, ctx.has_b = cell, (b_ih is not None, b_hh is not None)
        return load().gru_update(x, h, w_ih, w_hh, b_ih, b_hh, cell)

    @staticmethod
    def backward(ctx, dh_out):
        x, h, w_ih, w_hh, *bs = ctx.saved_tensors
        b_ih = bs.pop(0) if ctx.has_b[0] else None
        b_hh = bs.pop(0) if ctx.has_b[1] else None
        need = [int(n) for n in ctx.needs_input_grad[:6]]
        need[4], need[5] = need[4] and int(ctx.has_b[0]), need[5] and int(ctx.has_b[1])
        outs = load().gru_update_bwd(dh_out.contiguous(), x, h, w_ih, w_hh, b_ih, b_hh, ctx.cell, need)
        return _grads(outs, need) + (None,)


def memory_cell(x, h, w_ih, w_hh, b_ih=None, b_hh=None, cell="gru"):
    """TGNMemory.memory_updater (memory_module.py:70-78): torch.nn.GRUCell (cell 'gru' / 0) or RNNCell with tanh
    ('rnn' / 1) of x [M, d_in] and h [M, D] with torch's parameter layout; gradients flow to every tensor."""
    cell = {"gru": 0, "rnn": 1}.get(cell, cell)
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    return _MemoryCell.apply(c(x), c(h), c(w_ih), c(w_hh), c(b_ih), c(b_hh), int(cell))


class _LinkPredictor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_src, z_dst, w_src, b_src, w_dst, b_dst, w_out, b_out, sigmoid):
        ctx.save_for_backward(z_src, z_dst, w_src, w_dst, w_out, b_out, *(b for b in (b_src, b_dst) if b is not None))
        ctx.sigmoid, ctx.has_b = sigmoid, (b_src is not None, b_dst is not None)
        return load().predictor(z_src, z_dst, w_src, b_src, w_dst, b_dst, w_out, b_out, sigmoid)

    @staticmethod
    def backward(ctx, dout):
        z_src, z_dst, w_src, w_dst, w_out, b_out, *bs = ctx.saved_tensors
        b_src = bs.pop(0) if ctx.has_b[0] else None
        b_dst = bs.pop(0) if ctx.has_b[1] else None
        n = [int(v) for v in ctx.needs_input_grad[:8]]   # inputs: z_src z_dst w_src b_src w_dst b_dst w_out b_out
        n[3], n[5] = n[3] and int(ctx.has_b[0]), n[5] and int(ctx.has_b[1])
        # the op's order: dz_src dz_dst dw_src db_src dw_dst db_dst dw_out db_out (the same)
        outs = load().predictor_bwd(dout.contiguous().view(-1), z_src, z_dst, w_src, b_src, w_dst, b_dst, w_out, b_out,
                                    ctx.sigmoid, n)
        return _grads(outs, n) + (None,)


def link_predictor(z_src, z_dst, w_src, b_src, w_dst, b_dst, w_out, b_out, sigmoid=True):
    """LinkPredictor (decoder.py:12-27; sigmoid) / EdgePredictor (model_utils.py:165-195; logits, z_dst rows a
    multiple of z_src rows: row i pairs with source i mod B).  Returns [M, 1]; gradients flow to every tensor
    (z_src's is summed over the rows that share it)."""
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    return _LinkPredictor.apply(c(z_src), c(z_dst), c(w_src), c(b_src), c(w_dst), c(b_dst), c(w_out), c(b_out),
                                bool(sigmoid))


def _ragged(pair, n_src, dev, what, validate, need_sorted):
    """(ptr, values) as contiguous int64 device tensors and the longest segment (None without `validate`).
    validate: ONE host read checks ptr[0] == 0, ptr non-decreasing, ptr[-1] == len(values) and (need_sorted) every
    segment ascending; ValueError otherwise."""
    ptr, vals = pair
    ptr = torch.as_tensor(ptr).to(dev, torch.long).contiguous().view(-1)
    vals = torch.as_tensor(vals).to(dev, torch.long).contiguous().view(-1)
    if ptr.numel() != n_src + 1:
        raise ValueError(f"link_topk: {what} ptr must have n_src + 1 = {n_src + 1} entries, got {ptr.numel()}")
    if not validate:
        return ptr, vals, None
    nnz = vals.numel()
    lens = ptr[1:] - ptr[:-1]
    ok_ptr = (ptr[0] == 0) & (ptr[-1] == nnz) & (lens >= 0).all()
    ok_sorted = torch.ones((), dtype=torch.bool, device=dev)
    if need_sorted and nnz > 1:
        start = torch.zeros(nnz + 1, dtype=torch.bool, device=dev)
        start[ptr.clamp(0, nnz)] = True            # a descent across a segment boundary is none
        ok_sorted = ~((vals[1:] < vals[:-1]) & ~start[1:nnz]).any()
    longest = lens.max() if n_src else torch.zeros((), dtype=torch.long, device=dev)
    ok_ptr, ok_sorted, longest = torch.stack([ok_ptr.long(), ok_sorted.long(), longest]).tolist()
    if not ok_ptr:
        raise ValueError(f"link_topk: {what} ptr must start at 0, not decrease and end at len(values) = {nnz}")
    if not ok_sorted:
        raise ValueError(f"link_topk: every {what} segment must be ascending")
    return ptr, vals, int(longest)


@torch.no_grad()
def link_topk(z_src, z_cand, w_src, b_src, w_dst, b_dst, w_out, b_out, k, sigmoid=True, return_scores=False,
              cand_key=None, src_key=None, exclude=None, lists=None, validate=True, max_len=None):
    """The k best candidates of every source under LinkPredictor (decoder.py:12-27), scored over all n_src x n_cand
    pairs and selected in the same kernel (tgnx_link_predictor_topk): no [n_src * n_cand, d] operand, no score
    matrix handed to torch.topk.  Returns (val [n_src, k], idx [n_src, k]) and, with return_scores, the logits
    [n_src, n_cand] the selection compared.  idx holds positions into z_cand, ordered by larger logit, equal logits
    by lower position; val the logits, or their sigmoid (sigmoid=True); slots past n_cand hold idx -1 and val -inf
    (0 with sigmoid).  The selection is always on the logit.  Inference only: no autograd.

    Per-source exclusions (tgnx_link_predictor_topk_filtered; any of cand_key, src_key, exclude given): a candidate's
    key is cand_key[c] (int64 [n_cand]; default its position); it is left out for source q when the key equals
    src_key[q] (int64 [n_src]) or occurs in q's segment of exclude = (ptr [n_src + 1], keys), each segment ascending.
    Excluded pairs are never selected (padding when fewer than k remain); the returned logits are unmasked.

    A candidate list per source (tgnx_link_predictor_topk_lists; lists = (ptr [n_src + 1], positions into z_cand)):
    returns (val, idx, slot[, logits [nnz]]) with slot the entry's offset in its list and equal logits ordered by
    lower slot; an entry < 0 is skipped, one >= n_cand too (NaN in logits).  max_len: an upper bound on a list's
    length (default: the longest list when validated, else len(positions)).  Not combined with the exclusions:
    mask an entry by writing -1.

    validate: one host read per ragged argument checks ptr[0] == 0, ptr non-decreasing, ptr[-1] == len(values) and,
    for exclude, ascending segments (ValueError).  Without it the kernels still keep every access inside the arrays."""
    c = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    if cand_key is None and src_key is None and exclude is None and lists is None:
        val, idx, logits = load().predictor_topk(c(z_src), c(z_cand), c(w_src), c(b_src), c(w_dst), c(b_dst), c(w_out),
                                                 c(b_out), int(k), bool(sigmoid), bool(return_scores))
        return (val, idx, logits) if return_scores else (val, idx)
    dev, n_src = z_src.device, z_src.size(0)
    key = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.long).contiguous().view(-1)  # noqa: E731
    if lists is not None:
        if cand_key is not None or src_key is not None or exclude is not None:
            raise ValueError("link_topk: lists is not combined with cand_key / src_key / exclude (mask entries with -1)")
        ptr, pos, longest = _ragged(lists, n_src, dev, "lists", validate, need_sorted=False)
        if max_len is None:
            max_len = pos.numel() if longest is None else longest
        val, idx, slot, logits, _ = load().predictor_topk_lists(
            c(z_src), c(z_cand), c(w_src), c(b_src), c(w_dst), c(b_dst), c(w_out), c(b_out), int(k), bool(sigmoid),
            bool(return_scores), ptr, pos, int(max_len))
        return (val, idx, slot, logits) if return_scores else (val, idx, slot)
    ptr = keys = None
    if exclude is not None:
        ptr, keys, _ = _ragged(exclude, n_src, dev, "exclude", validate, need_sorted=True)
    val, idx, logits = load().predictor_topk_filtered(
        c(z_src), c(z_cand), c(w_src), c(b_src), c(w_dst), c(b_dst), c(w_out), c(b_out), int(k), bool(sigmoid),
        bool(return_scores), key(cand_key), key(src_key), ptr, keys)
    return (val, idx, logits) if return_scores else (val, idx)


@torch.no_grad()
def link_rank(z_src, z_cand, w_src, b_src, w_dst, b_dst, w_out, b_out, target, n_count=None, cand_key=None,
              src_key=None, exclude=None, validate=True):
    """Where source q's true destination z_cand[target[q]] stands among the first n_count rows of z_cand (default:
    all) under LinkPredictor (tgnx_link_predictor_rank): no [n_src, n_cand] logits, no selection.  Returns
    (rank float64 [n_src], gt, eq, n int64 [n_src], tlogit float32 [n_src]): with the keys and exclusions of
    link_topk's filtered form, a candidate is compared when its key is not the target's, not src_key[q], not in q's
    segment of exclude, and its logit is not NaN; gt / eq count the compared logits above / equal to the target's
    (tlogit, the bits of link_topk's logits[q, target[q]]), n all of them, and rank = 1 + gt + eq / 2 (TGB's
    convention).  The target is never excluded.  A target outside [0, n_cand) or a NaN tlogit: rank NaN, gt = eq = 0.
    validate: the one host read link_topk makes for exclude.  Inference only: no autograd."""
    c = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    dev, n_src = z_src.device, z_src.size(0)
    key = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.long).contiguous().view(-1)  # noqa: E731
    ptr = keys = None
    if exclude is not None:
        ptr, keys, _ = _ragged(exclude, n_src, dev, "exclude", validate, need_sorted=True)
    gt, eq, n, tlogit = load().predictor_rank(
        c(z_src), c(z_cand), c(w_src), c(b_src), c(w_dst), c(b_dst), c(w_out), c(b_out), key(target),
        z_cand.size(0) if n_count is None else int(n_count), key(cand_key), key(src_key), ptr, keys)
    rank = torch.add(gt, eq.double(), alpha=0.5).add_(1.0)
    return rank.masked_fill_(torch.isnan(tlogit), float("nan")), gt, eq, n, tlogit


def check_link_loo_args(z_shape, loo_shape, n_count, n_src, n_dst) -> tuple:
    """The shapes ops.link_loo takes: z [n, d], loo_z [n, K, d] with 1 <= K <= 64, count [n], src_row and dst_row of
    one length P.  Returns (n, K, P); ValueError otherwise.  (Host arithmetic only: no device, no library.)"""
    z_shape, loo_shape = tuple(z_shape), tuple(loo_shape)
    if len(z_shape) != 2 or len(loo_shape) != 3 or loo_shape[0] != z_shape[0] or loo_shape[2] != z_shape[1]:
        raise ValueError(f"link_loo: z must be [n, d] and loo_z [n, K, d], got {z_shape} and {loo_shape}")
    n, K = z_shape[0], loo_shape[1]
    if not 1 <= K <= 64:
        raise ValueError(f"link_loo: loo_z must hold 1 <= K <= 64 rows per node, got {K}")
    if n_count != n:
        raise ValueError(f"link_loo: count must have n = {n} entries, got {n_count}")
    if n_src != n_dst:
        raise ValueError(f"link_loo: {n_src} source rows for {n_dst} destination rows")
    return n, K, n_src


@torch.no_grad()
def link_loo(z, loo_z, count, src_row, dst_row, w_src, b_src, w_dst, b_dst, w_out, b_out):
    """Leave-one-out link logits (tgnx_link_predictor_loo, csrc/tgnx_explain.hip).  z [n, d] and loo_z [n, K, d] hold
    the embedding and the K leave-one-out embeddings of n unique nodes (TgnEngine's tgnx_tgn_explain outputs), count
    [n] how many of a node's K rows exist; pair p names rows src_row[p] and dst_row[p].  Returns (base [P], src_logit
    [P, K], dst_logit [P, K], status [1] int64): the pair's LinkPredictor logit, the logit with the source's embedding
    replaced by its row j (the destination at its full embedding), and the converse — each side varied alone also when
    both name one node; an entry past the varied node's count holds base's bits.  Every unique row is projected once
    (four GEMMs), then each logit is one sequential fma chain: its bits do not depend on the order of the pairs.  A row
    index outside [0, n) gives NaN outputs for its pair and status = 1; it is never dereferenced, and no host read
    checks it here.  Inference only: no autograd."""
    dev = z.device
    idx = lambda t: torch.as_tensor(t).to(dev, torch.long).contiguous().view(-1)  # noqa: E731
    c = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    src_row, dst_row = idx(src_row), idx(dst_row)
    count = torch.as_tensor(count).to(dev, torch.int32).contiguous().view(-1)
    check_link_loo_args(z.shape, loo_z.shape, count.numel(), src_row.numel(), dst_row.numel())
    return load().predictor_loo(c(z), c(loo_z), count, src_row, dst_row, c(w_src), c(b_src), c(w_dst), c(b_dst),
                                c(w_out).view(-1), c(b_out).view(-1))


KNN_METRICS = {"dot": 0, "cosine": 1}     # TGNX_KNN_DOT / TGNX_KNN_COSINE
TOPK_MAX = 128                            # TGNX_TOPK_MAX


def knn_metric(metric) -> int:
    """The C ABI's metric code of a metric name; ValueError for an unknown one."""
    if metric not in KNN_METRICS:
        raise ValueError(f"embed_knn: metric must be one of {sorted(KNN_METRICS)}, got {metric!r}")
    return KNN_METRICS[metric]


def knn_k(k) -> int:
    """k as an int inside the selection's range [1, TGNX_TOPK_MAX]; ValueError otherwise."""
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"embed_knn: k must be in [1, {TOPK_MAX}], got {k}")
    return k


@torch.no_grad()
def embed_knn(z_q, z_cand, k, metric="cosine", return_scores=False, cand_key=None, q_key=None, exclude=None,
              validate=True):
    """The k nearest candidate rows of every query row in embedding space (tgnx_embed_knn): z_q [n_q, D], z_cand
    [n_cand, D], D <= 256; metric "cosine" (rows scaled by 1 / sqrt(sum z^2); a zero row scores 0) or "dot".  All
    n_q x n_cand scores come from the f32 MFMA and are selected in the same kernel: no [n_q, n_cand] matrix handed to
    torch.topk.  Returns (val [n_q, k], idx [n_q, k]) and, with return_scores, the unmasked scores [n_q, n_cand] the
    selection compared.  idx holds positions into z_cand, ordered by larger score, equal scores by lower position; a
    NaN score is never selected; slots past the candidates hold idx -1 and val -inf.  A pair's score has the same
    bits whatever the other rows, their order and their number are.  Inference only: no autograd.

    Exclusions as link_topk's filtered form: a candidate's key is cand_key[c] (int64 [n_cand]; default its position);
    it is left out for query q when the key equals q_key[q] (int64 [n_q]: "not myself") or occurs in q's segment of
    exclude = (ptr [n_q + 1], keys), each segment ascending.  validate: one host read checks exclude's shape and
    order (ValueError); without it the kernel still keeps every access inside the arrays."""
    code, k = knn_metric(metric), knn_k(k)
    dev, n_q = z_q.device, z_q.size(0)
    key = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.long).contiguous().view(-1)  # noqa: E731
    ptr = keys = None
    if exclude is not None:
        ptr, keys, _ = _ragged(exclude, n_q, dev, "exclude", validate, need_sorted=True)
    val, idx, scores = load().embed_knn(z_q.detach().contiguous(), z_cand.detach().contiguous(), code, k,
                                        bool(return_scores), key(cand_key), key(q_key), ptr, keys)
    return (val, idx, scores) if return_scores else (val, idx)


class _TimeEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, w, b):
        ctx.save_for_backward(t, w, b)
        return load().time_encode(t, w, b)

    @staticmethod
    def backward(ctx, dout):
        t, w, b = ctx.saved_tensors
        _, nw, nb = ctx.needs_input_grad
        if not (nw or nb):
            return None, None, None
        dw, db = load().time_encode_bwd(dout.contiguous(), t, w, b)
        return None, (dw if nw else None), (db if nb else None)


def time_encode(t, w, b):
    """TimeEncoder: cos(w t + b) [n, D] of t [n] (fp32), w [D] or [D, 1], b [D]; the argument is the fused
    kernels' fmaf(w, t, b) with their exact reduction.  t is data: it gets no gradient."""
    return _TimeEncode.apply(t.contiguous(), w.contiguous(), b.contiguous())


class _TimeEmbedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rel_t, w, b):
        ctx.save_for_backward(x, rel_t, w, b)
        return load().time_embedding(x, rel_t, w, b)

    @staticmethod
    def backward(ctx, dout):
        x, rel_t, w, b = ctx.saved_tensors
        nx, _, nw, nb = ctx.needs_input_grad
        dx, dw, db = load().time_embedding_bwd(dout.contiguous(), x, rel_t, w, b, bool(nx))
        return (dx if nx else None), None, (dw if nw else None), (db if nb else None)


def time_embedding(x, rel_t, w, b):
    """TimeEmbedding (emb_module.py:48-50): x (1 + w rel_t + b) for x [n, D], rel_t [n] (fp32), w [D] or [D, 1],
    b [D]; gradients flow to x, w, b."""
    return _TimeEmbedding.apply(x.contiguous(), rel_t.contiguous(), w.contiguous(), b.contiguous())


class _AggregateLast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, index, t, dim_size):
        out, argmax = load().msg_agg_last(msg, index, t, dim_size)
        ctx.save_for_backward(argmax)
        ctx.n_msg = msg.size(0)
        return out

    @staticmethod
    def backward(ctx, dout):
        (argmax,) = ctx.saved_tensors
        return load().msg_agg_last_bwd(dout.contiguous(), argmax, ctx.n_msg), None, None, None


def aggregate_last(msg, index, t, dim_size):
    """LastAggregator (msg_agg.py:15-21): per row of `index` the message with the largest t (the first on a tie),
    zeros for a row without messages.  The gradient scatters back to the chosen messages."""
    return _AggregateLast.apply(msg.contiguous(), index.contiguous(), t.contiguous(), int(dim_size))


class _AggregateMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, index, dim_size):
        ctx.save_for_backward(index)
        return load().msg_agg_mean(msg, index, dim_size)

    @staticmethod
    def backward(ctx, dout):
        (index,) = ctx.saved_tensors
        return load().msg_agg_mean_bwd(dout.contiguous(), index), None, None


def aggregate_mean(msg, index, dim_size):
    """MeanAggregator (msg_agg.py:24-26): per row of `index` the mean of its messages, zeros for an empty row."""
    return _AggregateMean.apply(msg.contiguous(), index.contiguous(), int(dim_size))


class _BuildMessages(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, b, slot, n_s, log_src, log_dst, log_t, log_raw, fill, memory, last_update, emb, assoc, stamp,
                n_id, emb_flags):
        buf, t_rel = load().memstore_build_msg(slot, n_s, log_src, log_dst, log_t, log_raw, fill, memory, last_update,
                                               w, b, emb, assoc, stamp, n_id, emb_flags)
        ctx.save_for_backward(t_rel, w, b)
        ctx.te0 = buf.size(1) - b.numel()
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        t_rel, w, b = ctx.saved_tensors
        nw, nb = ctx.needs_input_grad[:2]
        dw = db = None
        if nw or nb:
            dw, db = load().time_encode_bwd(dbuf[:, ctx.te0:].contiguous(), t_rel, w, b)
        return (dw if nw else None, db if nb else None) + (None,) * 14


def build_messages(w, b, slot, n_s, log_src, log_dst, log_t, log_raw, fill, memory, last_update, emb=None, assoc=None,
                   stamp=None, n_id=None, emb_flags=0):
    """The message inputs of TGNMemory._compute_msg (memory_module.py:193-207) for gathered store slots, one
    buffer [n_msg, 2 D + d + T] = [memory[src] | memory[dst] | raw_msg | cos(w t_rel + b)] (tgnx_memstore_build_msg).
    The memory, raw-message and (DyRep) embedding columns are data; the time-encoding columns carry the gradient
    to w and b through time_encode_bwd with the saved t_rel."""
    return _BuildMessages.apply(w.contiguous(), b.contiguous(), slot, int(n_s), log_src, log_dst, log_t, log_raw,
                                int(fill), memory, last_update, emb, assoc, stamp, n_id, int(emb_flags))


# ---------------------------------------------------------------------- node property prediction (tgnx_nodeprop.hip)
NODE_MAX_K = 128                          # TGNX_NODE_MAX_K
_ndcg_cum = {}


def ndcg_cum(k: int):
    """cum[j] = sum of the first j NDCG discounts 1 / log2(r + 1), j = 0..k, in float64 on the host (the device never
    evaluates log2): a plain list."""
    import math
    cum = [0.0]
    for r in range(1, int(k) + 1):
        cum.append(cum[-1] + 1.0 / math.log2(r + 1))
    return cum


def _cum_on(k: int, device):
    k = int(k)
    if not 1 <= k <= NODE_MAX_K:
        raise ValueError(f"ndcg: k must be in [1, {NODE_MAX_K}], got {k}")
    key = (k, str(device))
    if key not in _ndcg_cum:
        _ndcg_cum[key] = torch.tensor(ndcg_cum(k), dtype=torch.float64, device=device)
    return _ndcg_cum[key]


class _NodePredictor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, w1, b1, w2, b2):
        need_h = any(ctx.needs_input_grad)
        logits, h = load().node_predictor(z, w1, b1, w2, b2, need_h)
        if need_h:
            ctx.save_for_backward(z, h, w1, w2)
        ctx.has_b = (b1 is not None, b2 is not None)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        z, h, w1, w2 = ctx.saved_tensors
        nz, nw1, nb1, nw2, nb2 = (int(v) for v in ctx.needs_input_grad)
        need = [nz, nw1, nb1 and int(ctx.has_b[0]), nw2, nb2 and int(ctx.has_b[1])]
        dz, dw1, db1, dw2, db2 = _grads(load().node_predictor_bwd(dlogits.contiguous(), z, h, w1, w2, need), need)
        return dz, dw1, db1, dw2, db2


def node_predictor(z, w1, b1, w2, b2):
    """NodePredictor (decoder.py:30-41): logits [M, C] = W2 relu(W1 z + b1) + b2 for z [M, D], w1 [D, D], w2 [C, D]
    (D <= 128, C <= 4096), two launches of the f32 MFMA GEMM with bias and ReLU in the epilogues; the hidden rows are
    kept only when a gradient is needed.  Gradients flow to every tensor (dz too, so a composed model trains through
    the head)."""
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    return _NodePredictor.apply(c(z), c(w1), c(b1), c(w2), c(b2))


class _NodeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, y, k):
        need_grad = ctx.needs_input_grad[0]
        want_ndcg = k is not None
        cum = _cum_on(k if want_ndcg else 1, logits.device)
        mean, _rows, dl, nd = load().node_loss_ndcg(logits, y, cum, int(k) if want_ndcg else 1, True, need_grad,
                                                    want_ndcg)
        if need_grad:
            ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(nd)
        return mean, nd

    @staticmethod
    def backward(ctx, g, _gnd):
        (dl,) = ctx.saved_tensors
        if float(g) != 1.0:            # (loss.backward() passes 1: the saved dlogits are the gradient as they are)
            dl = dl * g
        return dl, None, None


def soft_cross_entropy(logits, y):
    """Mean over rows of the soft-target cross-entropy of logits [M, C] against dense targets y [M, C] (>= 0, any row
    sum): torch.nn.functional.cross_entropy(logits, y) with probability targets, from the row kernel
    (tgnx_node_loss_ndcg).  The forward already wrote dlogits (scaled by 1 / M); backward returns them, multiplied by
    the incoming gradient only when that is not 1.  y is data: no gradient.  An empty batch gives 0."""
    return _NodeLoss.apply(logits.contiguous(), y.contiguous(), None)[0]


@torch.no_grad()
def ndcg_at_k(logits, y, k=10):
    """NDCG@k of every row, float64 [M]: sklearn's ndcg_score(y, logits, k=k) with its tie averaging (tied scores
    share the mean discount of the ranks they span), 0 for a row without a positive target.  No autograd."""
    return load().node_loss_ndcg(logits.detach().contiguous(), y.contiguous(), _cum_on(k, logits.device), int(k),
                                 False, False, True)[3]


def node_loss_ndcg(logits, y, k=10):
    """(soft_cross_entropy(logits, y), ndcg_at_k(logits, y, k)) from ONE pass of the row kernel over the logits (the
    mean of the row losses is a second, one-workgroup launch): what the train_node / test_node loops call.  The loss
    carries autograd as soft_cross_entropy's; the NDCG rows do not."""
    return _NodeLoss.apply(logits.contiguous(), y.contiguous(), int(k))
