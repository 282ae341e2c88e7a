"""tgnx.nn — the reference's `modules/` package as trainable torch.nn.Modules over the HIP operators.

Each module keeps the constructor arguments and state_dict() keys of the module it stands for, so a state dict of
the reference model (or of the restatements in oracle/tgn_ref.py) loads with strict=True, and its forward runs the
autograd functions of tgnx/ops.py (HIP kernels forward and backward; no eager-PyTorch arithmetic on the hot path):

    TimeEncoder(out_channels)                          [ext] torch_geometric TimeEncoder (modules/time_enc.py)
    IdentityMessage(raw_msg_dim, memory_dim, time_dim) modules/msg_func.py:12-18
    LastAggregator / MeanAggregator                    modules/msg_agg.py:15-26
    MemoryCell(input, hidden, cell='gru' | 'rnn')      TGNMemory.memory_updater, memory_module.py:57,70-78
    TransformerConv(in, out, heads, dropout, edge_dim) [ext] torch_geometric TransformerConv (concat, root weight)
    GraphAttentionEmbedding(in, out, msg_dim, time_enc)  modules/emb_module.py:11-29
    TimeEmbedding(in, out)                             modules/emb_module.py:32-52 (JODIE's projection)
    LinkPredictor(in_channels)                         modules/decoder.py:12-27
    NodePredictor(in_dim, out_dim)                     modules/decoder.py:30-41 (TGB node property prediction)
    TGNMemory(num_nodes, raw_msg_dim, memory_dim, time_dim, message_module, aggregator_module,
              memory_updater_cell='gru')               modules/memory_module.py:25-215
    DyRepMemory(..., memory_updater_type, use_src_emb_in_msg=False, use_dst_emb_in_msg=False)
                                                       modules/memory_module.py:218-421

Constructing a module (the two memories and their stores included) and calling state_dict() needs neither a GPU
nor the built library; forward, update_state, train(False) and message_store need both (the module and its inputs
on the HIP device).  Plumbing stays in torch: torch.cat, the gathers x[index], the row writes memory[n_id] = ...,
the edge sort and the stable sort of a stored batch's node ids.  A gather's backward is torch's index_add, the one
part of a composed step whose summation order is not fixed.  The memories keep their message stores on the device
(csrc/tgnx_memstore.hip): putting a batch, gathering the stored events of a node set and building the message rows
are HIP launches with no per-node host work.
"""
from __future__ import annotations

import copy
import math

import torch
from torch import nn

from . import ops


class TimeEncoder(nn.Module):
    """cos(Linear(1, D)(t)): parameters lin.weight [D, 1], lin.bias [D]."""

    def __init__(self, out_channels: int):
        super().__init__()
        self.out_channels = out_channels
        self.lin = nn.Linear(1, out_channels)

    def reset_parameters(self):
        self.lin.reset_parameters()

    def forward(self, t):
        return ops.time_encode(t.reshape(-1).to(self.lin.weight.dtype), self.lin.weight, self.lin.bias)


class IdentityMessage(nn.Module):
    def __init__(self, raw_msg_dim: int, memory_dim: int, time_dim: int):
        super().__init__()
        self.out_channels = raw_msg_dim + 2 * memory_dim + time_dim

    def forward(self, z_src, z_dst, raw_msg, t_enc):
        return torch.cat([z_src, z_dst, raw_msg, t_enc], dim=-1)


class LastAggregator(nn.Module):
    def forward(self, msg, index, t, dim_size: int):
        return ops.aggregate_last(msg, index, t, dim_size)


class MeanAggregator(nn.Module):
    def forward(self, msg, index, t, dim_size: int):
        return ops.aggregate_mean(msg, index, dim_size)


class MemoryCell(nn.Module):
    """torch.nn.GRUCell (cell='gru') or RNNCell with tanh ('rnn') with their parameter names (weight_ih, weight_hh,
    bias_ih, bias_hh) and initialisation: a TGNMemory.memory_updater state dict loads into it."""

    def __init__(self, input_size: int, hidden_size: int, cell: str = "gru", bias: bool = True):
        super().__init__()
        if cell not in ("gru", "rnn"):
            raise ValueError("Memory updater can be either 'gru' or 'rnn'.")
        self.input_size, self.hidden_size, self.cell = input_size, hidden_size, cell
        g = (3 if cell == "gru" else 1) * hidden_size
        self.weight_ih = nn.Parameter(torch.empty(g, input_size))
        self.weight_hh = nn.Parameter(torch.empty(g, hidden_size))
        if bias:
            self.bias_ih = nn.Parameter(torch.empty(g))
            self.bias_hh = nn.Parameter(torch.empty(g))
        else:
            self.register_parameter("bias_ih", None)
            self.register_parameter("bias_hh", None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.hidden_size) if self.hidden_size > 0 else 0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def forward(self, x, h):
        return ops.memory_cell(x, h, self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh, self.cell)


class TransformerConv(nn.Module):
    """torch_geometric.nn.TransformerConv(in, out, heads, dropout=, edge_dim=) with concat=True, beta=False,
    root_weight=True: out_i = Σ_j α_ij (W_v x_j + W_e e_ij) + W_skip x_i, α the per-destination softmax of
    (W_q x_i)·(W_k x_j + W_e e_ij) / sqrt(out).

    Attention dropout (training mode, dropout > 0) is applied to α after the softmax under the engine's counter-based
    mask (ops.edge_attention), a function of a seed and not of torch's RNG.  The module must therefore know a seed:
    pass forward(..., seed=) per call, or call set_dropout_seed(base) once, after which the nb-th training forward
    uses ops.step_seed(base, nb) as the engine's nb-th batch does.  Without either, a training forward at
    dropout > 0 raises NotImplementedError; eval() or dropout=0.0 runs without a seed.  The mask's keys default to
    the row of x for a destination and the edge's column in the caller's edge_index for an edge (so an edge's mask
    does not depend on how the list was ordered); dst_key [N] / edge_key [E] (int64, e.g. node ids and event ids)
    replace them."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, dropout: float = 0.0,
                 edge_dim: int | None = None):
        super().__init__()
        if edge_dim is None:
            raise ValueError("TransformerConv: edge_dim is required (the TGN embedding always has edge features)")
        self.in_channels, self.out_channels, self.heads, self.dropout, self.edge_dim = (
            in_channels, out_channels, heads, dropout, edge_dim)
        self.lin_key = nn.Linear(in_channels, heads * out_channels)
        self.lin_query = nn.Linear(in_channels, heads * out_channels)
        self.lin_value = nn.Linear(in_channels, heads * out_channels)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        self.lin_skip = nn.Linear(in_channels, heads * out_channels)
        # plain attributes (not buffers: state_dict() keeps the reference's keys)
        self._drop_base, self._drop_calls = None, 0

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge, self.lin_skip):
            lin.reset_parameters()

    def set_dropout_seed(self, base_seed: int | None):
        """Enable attention dropout in training forwards that pass no seed: the nb-th such forward from now on
        (nb = 1, 2, ...) uses ops.step_seed(base_seed, nb).  None switches back to raising."""
        self._drop_base = None if base_seed is None else int(base_seed)
        self._drop_calls = 0

    def take_dropout_seed(self):
        """What a training forward without an explicit seed does first, in host arithmetic only: advance the call
        counter and return ops.step_seed(base, counter); None (and no advance) when no base seed is set."""
        if self._drop_base is None:
            return None
        self._drop_calls += 1
        return ops.step_seed(self._drop_base, self._drop_calls)

    def forward(self, x, edge_index, edge_attr, *, seed=None, dst_key=None, edge_key=None):
        drop = self.training and self.dropout > 0
        if drop and seed is None:
            seed = self.take_dropout_seed()
            if seed is None:
                raise NotImplementedError(
                    "tgnx.nn.TransformerConv: attention dropout in training mode needs a seed (the mask is a "
                    "counter-based hash, not torch's RNG): pass forward(..., seed=) or call set_dropout_seed(base) "
                    "once; or call eval() / construct with dropout=0.0 to run without dropout")
        n = x.size(0)
        src, dst = edge_index[0], edge_index[1]                     # flow source_to_target
        q = ops.linear(x, self.lin_query.weight, self.lin_query.bias)
        k = ops.linear(x, self.lin_key.weight, self.lin_key.bias)
        v = ops.linear(x, self.lin_value.weight, self.lin_value.bias)
        e = ops.linear(edge_attr, self.lin_edge.weight, None)
        # destination i's edges as the contiguous rows [indptr[i], indptr[i+1]), in their given order
        dst_sorted, perm = torch.sort(dst, stable=True)
        indptr = torch.zeros(n + 1, dtype=torch.long, device=x.device)
        indptr[1:] = torch.cumsum(torch.bincount(dst_sorted, minlength=n), 0)
        j = src[perm]
        if drop:  # an edge's key: the caller's, or its column in the caller's edge_index (not its sorted position)
            out, _ = ops.edge_attention(q, k[j], v[j], e[perm], indptr, self.heads, dropout=self.dropout, seed=seed,
                                        dst_key=dst_key, edge_key=perm if edge_key is None else edge_key[perm])
        else:
            out, _ = ops.edge_attention(q, k[j], v[j], e[perm], indptr, self.heads)
        return out + ops.linear(x, self.lin_skip.weight, self.lin_skip.bias)


class GraphAttentionEmbedding(nn.Module):
    """modules/emb_module.py:11-29: one TransformerConv (2 heads of out_channels // 2) over edge attributes
    [time_enc(last_update[src] - t), msg].  `dropout` is the reference's fixed 0.1; training with it needs a
    seed, per call or through set_dropout_seed (see TransformerConv), and seed / dst_key / edge_key pass through."""

    def __init__(self, in_channels: int, out_channels: int, msg_dim: int, time_enc: nn.Module, dropout: float = 0.1):
        super().__init__()
        self.time_enc = time_enc
        edge_dim = msg_dim + time_enc.out_channels
        self.conv = TransformerConv(in_channels, out_channels // 2, heads=2, dropout=dropout, edge_dim=edge_dim)

    def set_dropout_seed(self, base_seed: int | None):
        self.conv.set_dropout_seed(base_seed)

    def forward(self, x, last_update, edge_index, t, msg, *, seed=None, dst_key=None, edge_key=None):
        rel_t = last_update[edge_index[0]] - t
        rel_t_enc = self.time_enc(rel_t.to(x.dtype))
        edge_attr = torch.cat([rel_t_enc, msg], dim=-1)
        return self.conv(x, edge_index, edge_attr, seed=seed, dst_key=dst_key, edge_key=edge_key)


class _NormalLinear(nn.Linear):
    """Linear initialised normal(0, 1 / sqrt(fan_in)) (JODIE's, as TGN's)."""

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weight.size(1))
        nn.init.normal_(self.weight, 0.0, stdv)
        if self.bias is not None:
            nn.init.normal_(self.bias, 0.0, stdv)


class TimeEmbedding(nn.Module):
    """JODIE's time projection (modules/emb_module.py:32-52): x (1 + Linear(1, out)(last_update - t))."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.embedding_layer = _NormalLinear(1, out_channels)

    def forward(self, x, last_update, t):
        rel_t = (last_update - t).to(x.dtype)
        return ops.time_embedding(x, rel_t, self.embedding_layer.weight, self.embedding_layer.bias)


class LinkPredictor(nn.Module):
    """modules/decoder.py:12-27: sigmoid(lin_final(relu(lin_src(z_src) + lin_dst(z_dst)))), [M, 1]."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.lin_src = nn.Linear(in_channels, in_channels)
        self.lin_dst = nn.Linear(in_channels, in_channels)
        self.lin_final = nn.Linear(in_channels, 1)

    def forward(self, z_src, z_dst):
        return ops.link_predictor(z_src, z_dst, self.lin_src.weight, self.lin_src.bias, self.lin_dst.weight,
                                  self.lin_dst.bias, self.lin_final.weight, self.lin_final.bias, sigmoid=True)

    def topk(self, z_src, z_cand, k, return_scores=False):
        """The k best rows of z_cand for every row of z_src: (val [n_src, k] sigmoid outputs, idx [n_src, k] positions
        into z_cand[, logits [n_src, n_cand]]), all pairs scored and selected in one fused kernel (ops.link_topk; the
        selection is on the logit, ties by lower position, -1 / 0 padding when k > n_cand).  No autograd."""
        return ops.link_topk(z_src, z_cand, self.lin_src.weight, self.lin_src.bias, self.lin_dst.weight,
                             self.lin_dst.bias, self.lin_final.weight, self.lin_final.bias, k, sigmoid=True,
                             return_scores=return_scores)

    def topk_filtered(self, z_src, z_cand, k, return_scores=False, *, cand_key=None, src_key=None, exclude=None,
                      lists=None, validate=True, max_len=None):
        """topk with ops.link_topk's per-source keywords forwarded: exclusions by key (cand_key, src_key, exclude =
        (ptr, keys)) return (val, idx[, logits]); a candidate list per source (lists = (ptr, positions)) returns
        (val, idx, slot[, ragged logits]).  With none of them given it is topk."""
        return ops.link_topk(z_src, z_cand, self.lin_src.weight, self.lin_src.bias, self.lin_dst.weight,
                             self.lin_dst.bias, self.lin_final.weight, self.lin_final.bias, k, sigmoid=True,
                             return_scores=return_scores, cand_key=cand_key, src_key=src_key, exclude=exclude,
                             lists=lists, validate=validate, max_len=max_len)

    def rank(self, z_src, z_cand, target, **kw):
        """Where z_cand[target[q]] stands for source q among the rows of z_cand: (rank [n_src] float64, gt, eq, n,
        tlogit), ops.link_rank with its keywords (n_count, cand_key, src_key, exclude, validate) forwarded.  No
        autograd."""
        return ops.link_rank(z_src, z_cand, self.lin_src.weight, self.lin_src.bias, self.lin_dst.weight,
                             self.lin_dst.bias, self.lin_final.weight, self.lin_final.bias, target, **kw)

    def loo(self, z, loo_z, count, src_row, dst_row):
        """Leave-one-out logits of the pairs (z[src_row[p]], z[dst_row[p]]): (base [P], src_logit [P, K], dst_logit
        [P, K], status [1]) — ops.link_loo with this predictor's parameters; z [n, d], loo_z [n, K, d] and count [n]
        per unique node.  No autograd."""
        return ops.link_loo(z, loo_z, count, src_row, dst_row, self.lin_src.weight, self.lin_src.bias,
                            self.lin_dst.weight, self.lin_dst.bias, self.lin_final.weight, self.lin_final.bias)


class NodePredictor(nn.Module):
    """modules/decoder.py:30-41: out(relu(lin_node(node_embed))), logits [M, out_dim] (no softmax, as the reference);
    in_dim <= 128, out_dim <= 4096.  ops.soft_cross_entropy / ops.node_loss_ndcg are its loss and metric."""

    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.lin_node = nn.Linear(in_dim, in_dim)
        self.out = nn.Linear(in_dim, out_dim)

    def forward(self, node_embed):
        return ops.node_predictor(node_embed, self.lin_node.weight, self.lin_node.bias, self.out.weight, self.out.bias)


class TGNMemory(nn.Module):
    """modules/memory_module.py:25-215 over a device message store (csrc/tgnx_memstore.hip).

    Submodules and buffers carry the reference's names (msg_s_module, msg_d_module — a deep copy —, aggr_module,
    time_enc, memory_updater; memory [N, D] f32, last_update [N] int64, _assoc [N] int64), so a reference state dict
    loads with strict=True.  The stores are non-persistent buffers (they follow .to(device) and stay out of the state
    dict, as the reference's dicts do): an append-only event log _log_src / _log_dst / _log_t int64[cap], _log_raw
    f32[cap, d] that holds each batch once, the node table _node_tab int64[4 N] {s_off, s_cnt, d_off, d_cnt} and the
    arena _arena int64[2 cap] of log slots.  The fill level is a host integer; the log grows geometrically;
    reset_state() and the flush of train(False) rewind it.  Dead entries are not compacted within an epoch.

    t and last_update are int64 (PyG's convention), raw_msg f32; t_rel = t - last_update[src] is taken in int64 and
    then cast.  A node's stored events keep batch order; messages are ordered [msg_s of n_id[0], n_id[1], ...;
    msg_d of n_id[0], ...]; LastAggregator's ties go to the first message in that order.  n_id must be
    free of duplicates, as in the reference's loop (forward's callers pass a unique() result).

    forward(n_id) reads one size from the device (the message count, to allocate the rows); the aggregation op
    keeps its own index check.  update_state's store update runs without any host synchronisation.
    `message_module` is called as (z_src, z_dst, raw_msg, t_enc) -> [n_msg, out_channels] on four column views of
    one buffer the build kernel writes; IdentityMessage takes that buffer as its output without a torch.cat.
    `aggregator_module` is called as (msg, index, t, dim_size)."""

    _FLUSH_CHUNK = 1 << 18  # train(False): nodes per memory(n_id) pass (bounds the [chunk, out_channels] rows)

    def __init__(self, num_nodes: int, raw_msg_dim: int, memory_dim: int, time_dim: int, message_module: nn.Module,
                 aggregator_module: nn.Module, memory_updater_cell: str = "gru", store_capacity: int = 4096):
        super().__init__()
        self.num_nodes, self.raw_msg_dim, self.memory_dim, self.time_dim = num_nodes, raw_msg_dim, memory_dim, time_dim
        self.use_src_emb_in_msg = self.use_dst_emb_in_msg = False
        self.msg_s_module = message_module
        self.msg_d_module = copy.deepcopy(message_module)
        self.aggr_module = aggregator_module
        self.time_enc = TimeEncoder(time_dim)
        self.memory_updater = MemoryCell(message_module.out_channels, memory_dim, memory_updater_cell)
        self.register_buffer("memory", torch.empty(num_nodes, memory_dim))
        self.register_buffer("last_update", torch.empty(num_nodes, dtype=torch.long))
        self.register_buffer("_assoc", torch.zeros(num_nodes, dtype=torch.long))
        cap =max(int(store_capacity), 1)
        for name in ("_log_src", "_log_dst", "_log_t"):
            self.register_buffer(name, torch.zeros(cap, dtype=torch.long), persistent=False)
        self.register_buffer("_log_raw", torch.zeros(cap, raw_msg_dim), persistent=False)
        self.register_buffer("_arena", torch.zeros(2 * cap, dtype=torch.long), persistent=False)
        self.register_buffer("_node_tab", torch.zeros(4 * num_nodes, dtype=torch.long), persistent=False)
        self.register_buffer("_store_bad", torch.zeros(1, dtype=torch.long), persistent=False)
        self._fill = 0
        self.reset_parameters()

    @property
    def device(self) -> torch.device:
        return self.time_enc.lin.weight.device

    def reset_parameters(self):
        for m in (self.msg_s_module, self.msg_d_module, self.aggr_module):
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()
        self.time_enc.reset_parameters()
        self.memory_updater.reset_parameters()
        self.reset_state()

    def reset_state(self):
        """memory = 0, last_update = 0, both stores empty, the arena rewound."""
        self.memory.zero_()
        self.last_update.zero_()
        self._reset_message_store()

    def _reset_message_store(self):
        self._node_tab.zero_()
        self._store_bad.zero_()
        self._fill = 0

    def detach(self):
        self.memory.detach_()

    def forward(self, n_id):
        if self.training:
            return self._get_updated_memory(n_id)
        return self.memory[n_id], self.last_update[n_id]

    def update_state(self, src, dst, t, raw_msg):
        self._update_state(src, dst, t, raw_msg, None, None)

    def _update_state(self, src, dst, t, raw_msg, embeddings, assoc):
        n_id = torch.cat([src, dst]).unique()
        if self.training:
            self._update_memory(n_id, embeddings, assoc)
            self._update_msg_store(src, dst, t, raw_msg)
        else:
            self._update_msg_store(src, dst, t, raw_msg)
            self._update_memory(n_id, embeddings, assoc)

    @torch.no_grad()
    def _update_memory(self, n_id, embeddings=None, assoc=None):
        memory, last_update = self._get_updated_memory(n_id, embeddings, assoc)
        self.memory[n_id] = memory
        self.last_update[n_id] = last_update

    def _gather(self, n_id):
        """(slot, owner, t [n_s + n_d], last_update [M], n_s): tgnx_memstore_count, the one size read,
        tgnx_memstore_gather."""
        ns = ops.load()
        totals, ws = ns.memstore_count(self._node_tab, n_id, self._store_bad)
        n_s, n_d, bad = totals.tolist()
        if bad:
            raise IndexError(f"TGNMemory: {bad} node ids outside [0, {self.num_nodes}) in n_id or in stored batches")
        slot, owner, t, lu = ns.memstore_gather(self._node_tab, self._arena, self._log_t, self._fill, n_id, n_s, n_d, ws)
        return slot, owner, t, lu, n_s

    def _get_updated_memory(self, n_id, embeddings=None, assoc=None):
        n_id = n_id.contiguous()
        M = n_id.numel()
        self._assoc[n_id] = torch.arange(M, device=n_id.device)
        slot, owner, t, last_update, n_s = self._gather(n_id)
        flags = 0
        if embeddings is not None:
            flags = int(self.use_src_emb_in_msg) | (int(self.use_dst_emb_in_msg) << 1)
        emb = (embeddings.detach().contiguous(), assoc.contiguous(), self._assoc, n_id) if flags else (None,) * 4
        buf = ops.build_messages(self.time_enc.lin.weight, self.time_enc.lin.bias, slot, n_s, self._log_src,
                                 self._log_dst, self._log_t, self._log_raw, self._fill, self.memory, self.last_update,
                                 *emb, emb_flags=flags)
        if isinstance(self.msg_s_module, IdentityMessage) and isinstance(self.msg_d_module, IdentityMessage):
            msg = buf
        else:
            D, d = self.memory_dim, self.raw_msg_dim
            cols = (buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:2 * D + d], buf[:, 2 * D + d:])
            msg = torch.cat([self.msg_s_module(*(c[:n_s] for c in cols)),
                             self.msg_d_module(*(c[n_s:] for c in cols))], dim=0)
        aggr = self.aggr_module(msg, owner, t, M)
        memory = self.memory_updater(aggr, self.memory[n_id])
        return memory, last_update

    @torch.no_grad()
    def _update_msg_store(self, src, dst, t, raw_msg):
        """_update_msg_store of both directions (memory_module.py:133-134): a stable sort of the batch's node ids,
        then one launch.  No host synchronisation."""
        B = src.numel()
        if B == 0:
            return
        if self._fill + B > self._log_src.numel():
            self._grow(self._fill + B)
        keys, perm = torch.sort(torch.stack([src, dst]), dim=1, stable=True)
        ops.load().memstore_put(src.contiguous(), dst.contiguous(), t.contiguous(), raw_msg.contiguous(), keys, perm,
                                self._fill, self._log_src, self._log_dst, self._log_t, self._log_raw, self._arena,
                                self._node_tab, self._store_bad)
        self._fill += B

    def _grow(self, need: int):
        """Geometric growth by plain reallocation (arena entries are absolute log slots: they survive the move)."""
        cap = self._log_src.numel()
        while cap < need:
            cap *= 2
        f = self._fill
        for name, n in (("_log_src", f), ("_log_dst", f), ("_log_t", f), ("_log_raw", f), ("_arena", 2 * f)):
            old = getattr(self, name)
            new = old.new_zeros((2 * cap if name == "_arena" else cap,) + tuple(old.shape[1:]))
            new[:n] = old[:n]
            setattr(self, name, new)

    @torch.no_grad()
    def message_store(self, direction: str = "s"):
        """(count [N] int64, src, dst, t, raw_msg): the stored events of direction 's' (a node's events as src) or
        'd' (as dst), concatenated in node order; as in the reference's stores `src` is the owning node in both."""
        if direction not in ("s", "d"):
            raise ValueError("direction must be 's' or 'd'")
        n_id = torch.arange(self.num_nodes, device=self._node_tab.device)
        slot, _, t, _, n_s = self._gather(n_id)
        tab = self._node_tab.view(self.num_nodes, 4)
        if direction == "s":
            sel, count = slot[:n_s], tab[:, 1].clone()
            return count, self._log_src[sel], self._log_dst[sel], t[:n_s], self._log_raw[sel]
        sel, count = slot[n_s:], tab[:, 3].clone()
        return count, self._log_dst[sel], self._log_src[sel], t[n_s:], self._log_raw[sel]

    def train(self, mode: bool = True):
        if self.training and not mode:
            # flush every node's store into memory (every row from the pre-flush state), then empty the stores
            N, C = self.num_nodes, self._FLUSH_CHUNK
            with torch.no_grad():
                rows = [self._get_updated_memory(torch.arange(i, min(i + C, N), device=self.memory.device))
                        for i in range(0, N, C)]
                if rows:
                    self.memory.copy_(torch.cat([r[0] for r in rows]) if len(rows) > 1 else rows[0][0])
                    self.last_update.copy_(torch.cat([r[1] for r in rows]) if len(rows) > 1 else rows[0][1])
            self._reset_message_store()
        return super().train(mode)


class DyRepMemory(TGNMemory):
    """modules/memory_module.py:218-421: TGNMemory with the updater cell named memory_updater_type and, with
    use_src_emb_in_msg / use_dst_emb_in_msg, update_state(..., embeddings, assoc) building its messages with
    embeddings[assoc[x]] in place of the memory row of a source / destination endpoint x that is in the batch's node
    set (:387-408).  Membership is tested on the device against the stamps in _assoc.  The embeddings are data: they
    enter under no_grad.  assoc must map every such x to a row of `embeddings`."""

    def __init__(self, num_nodes: int, raw_msg_dim: int, memory_dim: int, time_dim: int, message_module: nn.Module,
                 aggregator_module: nn.Module, memory_updater_type: str, use_src_emb_in_msg: bool = False,
                 use_dst_emb_in_msg: bool = False, store_capacity: int = 4096):
        super().__init__(num_nodes, raw_msg_dim, memory_dim, time_dim, message_module, aggregator_module,
                         memory_updater_type, store_capacity)
        self.use_src_emb_in_msg, self.use_dst_emb_in_msg = bool(use_src_emb_in_msg), bool(use_dst_emb_in_msg)

    def update_state(self, src, dst, t, raw_msg, embeddings=None, assoc=None):
        self._update_state(src, dst, t, raw_msg, embeddings, assoc)


__all__ = ["TimeEncoder", "IdentityMessage", "LastAggregator", "MeanAggregator", "MemoryCell", "TransformerConv",
           "GraphAttentionEmbedding", "TimeEmbedding", "LinkPredictor", "NodePredictor", "TGNMemory", "DyRepMemory"]
