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

Constructing a module and calling state_dict() needs neither a GPU nor the built library; forward needs both
(the parameters and inputs on the HIP device).  Plumbing stays in torch: torch.cat, the gathers x[index] and the
edge sort.  A gather's backward is torch's index_add, the one part of a composed step whose summation order is
not fixed.  A stateful TGNMemory with a device message store is not provided here (the fused engine owns one).
"""
from __future__ import annotations

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
    (W_q x_i)·(W_k x_j + W_e e_ij) / sqrt(out).  The attention ops apply no dropout: training mode with
    dropout > 0 raises NotImplementedError; eval() or dropout=0.0 runs."""

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

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge, self.lin_skip):
            lin.reset_parameters()

    def forward(self, x, edge_index, edge_attr):
        if self.training and self.dropout > 0:
            raise NotImplementedError(
                "tgnx.nn.TransformerConv: attention dropout is not implemented by the attention ops; call eval() "
                "or construct with dropout=0.0 to train without it")
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
        out, _ = ops.edge_attention(q, k[j], v[j], e[perm], indptr, self.heads)
        return out + ops.linear(x, self.lin_skip.weight, self.lin_skip.bias)


class GraphAttentionEmbedding(nn.Module):
    """modules/emb_module.py:11-29: one TransformerConv (2 heads of out_channels // 2) over edge attributes
    [time_enc(last_update[src] - t), msg].  `dropout` is the reference's fixed 0.1 (see TransformerConv)."""

    def __init__(self, in_channels: int, out_channels: int, msg_dim: int, time_enc: nn.Module, dropout: float = 0.1):
        super().__init__()
        self.time_enc = time_enc
        edge_dim = msg_dim + time_enc.out_channels
        self.conv = TransformerConv(in_channels, out_channels // 2, heads=2, dropout=dropout, edge_dim=edge_dim)

    def forward(self, x, last_update, edge_index, t, msg):
        rel_t = last_update[edge_index[0]] - t
        rel_t_enc = self.time_enc(rel_t.to(x.dtype))
        edge_attr = torch.cat([rel_t_enc, msg], dim=-1)
        return self.conv(x, edge_index, edge_attr)


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


__all__ = ["TimeEncoder", "IdentityMessage", "LastAggregator", "MeanAggregator", "MemoryCell", "TransformerConv",
           "GraphAttentionEmbedding", "TimeEmbedding", "LinkPredictor"]
