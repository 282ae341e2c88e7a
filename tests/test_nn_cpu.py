"""CPU checks of the trainable module layer (tgnx/nn.py, tgb-tgn-dgl_amd/modules/, the backward entry points of
csrc/tgnx_ops_bwd.hip): constructing the modules and reading their state dicts needs no GPU; their parameter
names and shapes are those of the oracle's restatements (oracle/tgn_ref.py, themselves pinned to the reference by
tests/golden/); the new torch ops are registered; the new C entry points check their arguments before any
device call."""
import ctypes

import numpy as np
import pytest
import torch


def _same_state(mine: torch.nn.Module, ref: torch.nn.Module):
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape, k
    mine.load_state_dict(b, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, b[k]), k


def test_time_encoder_state_dict_matches_oracle():
    from oracle.tgn_ref import RefTimeEncoder
    from tgnx.nn import TimeEncoder
    m = TimeEncoder(100)
    assert m.out_channels == 100
    assert m.lin.weight.shape == (100, 1) and m.lin.bias.shape == (100,)
    _same_state(m, RefTimeEncoder(100))


def test_transformer_conv_state_dict_matches_oracle():
    from oracle.tgn_ref import RefTransformerConv
    from tgnx.nn import TransformerConv
    m = TransformerConv(100, 50, heads=2, dropout=0.1, edge_dim=272)
    _same_state(m, RefTransformerConv(100, 50, 2, 0.1, 272))
    assert m.lin_edge.bias is None and m.lin_skip.bias is not None


def test_graph_attention_embedding_state_dict_matches_oracle():
    from oracle.tgn_ref import RefGraphAttentionEmbedding, RefTimeEncoder
    from tgnx.nn import GraphAttentionEmbedding, TimeEncoder
    m = GraphAttentionEmbedding(100, 100, 172, TimeEncoder(100))
    _same_state(m, RefGraphAttentionEmbedding(100, 100, 172, RefTimeEncoder(100)))
    assert m.conv.heads == 2 and m.conv.out_channels == 50 and m.conv.edge_dim == 272


def test_link_predictor_state_dict_matches_oracle():
    from oracle.tgn_ref import RefLinkPredictor
    from tgnx.nn import LinkPredictor
    _same_state(LinkPredictor(100), RefLinkPredictor(100))


@pytest.mark.parametrize("cell", ["gru", "rnn"])
def test_memory_cell_state_dict_matches_torch_cells(cell):
    from oracle.tgn_ref import RefTGNMemory
    from tgnx.nn import MemoryCell
    ref = torch.nn.GRUCell(472, 100) if cell == "gru" else torch.nn.RNNCell(472, 100)
    _same_state(MemoryCell(472, 100, cell), ref)
    # a TGNMemory's memory_updater state dict loads
    mem = RefTGNMemory(10, 172, 100, 100, "last", cell)
    _same_state(MemoryCell(mem.out_channels, 100, cell), mem.memory_updater)
    with pytest.raises(ValueError):
        MemoryCell(4, 4, "lstm")


def test_time_embedding_parameters_and_init():
    from tgnx.nn import TimeEmbedding
    torch.manual_seed(0)
    m = TimeEmbedding(100, 4000)
    sd = m.state_dict()
    assert list(sd.keys()) == ["embedding_layer.weight", "embedding_layer.bias"]
    assert sd["embedding_layer.weight"].shape == (4000, 1) and sd["embedding_layer.bias"].shape == (4000,)
    # normal(0, 1 / sqrt(fan_in)), fan_in = 1: unit variance (a default Linear(1, D) is uniform in [-1, 1], std 0.58)
    assert 0.9 < float(sd["embedding_layer.weight"].std()) < 1.1
    assert 0.9 < float(sd["embedding_layer.bias"].std()) < 1.1
    assert float(sd["embedding_layer.weight"].abs().max()) > 2.0


def test_identity_message_and_aggregators_have_no_parameters():
    from tgnx.nn import IdentityMessage, LastAggregator, MeanAggregator
    im = IdentityMessage(172, 100, 100)
    assert im.out_channels == 472
    assert not im.state_dict() and not LastAggregator().state_dict() and not MeanAggregator().state_dict()
    out = im(torch.zeros(3, 100), torch.ones(3, 100), torch.zeros(3, 172), torch.ones(3, 100))
    assert out.shape == (3, 472)


def test_modules_package_reexports_tgnx_nn():
    import tgnx.nn as tnn
    from modules.decoder import LinkPredictor
    from modules.emb_module import GraphAttentionEmbedding, TimeEmbedding
    from modules.msg_agg import LastAggregator, MeanAggregator
    from modules.msg_func import IdentityMessage
    from modules.time_enc import TimeEncoder
    assert LinkPredictor is tnn.LinkPredictor
    assert GraphAttentionEmbedding is tnn.GraphAttentionEmbedding and TimeEmbedding is tnn.TimeEmbedding
    assert LastAggregator is tnn.LastAggregator and MeanAggregator is tnn.MeanAggregator
    assert IdentityMessage is tnn.IdentityMessage and TimeEncoder is tnn.TimeEncoder
    import modules
    assert modules.MemoryCell is tnn.MemoryCell


NEW_OPS = ("col_sum", "gru_update_bwd", "predictor_bwd", "time_encode", "time_encode_bwd", "time_embedding",
           "time_embedding_bwd", "msg_agg_last_bwd", "msg_agg_mean_bwd")


def test_new_torch_ops_are_listed_and_registered():
    from tgnx import ops
    ns = ops.load()
    for name in NEW_OPS:
        assert name in ops.OPS, name
        assert hasattr(ns, name), name
    for fn in ("memory_cell", "link_predictor", "time_encode", "time_embedding", "aggregate_last", "aggregate_mean",
               "linear", "edge_attention"):
        assert callable(getattr(ops, fn)), fn


def test_transformer_conv_training_dropout_raises_before_any_device_work():
    from tgnx.nn import TransformerConv
    conv = TransformerConv(8, 4, heads=2, dropout=0.1, edge_dim=3).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.zeros(2, 8), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 3))


def _buf(n=64):
    a = np.zeros(n, dtype=np.float32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_backward_entry_points_check_arguments_before_any_device_call():
    """Each call fails in its argument check (host pointers are never touched; no HIP call is made)."""
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    rc = L.tgnx_memory_cell_bwd(2, 1, 4, 4, p, p, p, p, p, null, null, p, p, p, p, null, null, p, 1 << 20, null)
    assert rc != 0 and b"tgnx_memory_cell_bwd" in L.tgnx_last_error()
    rc = L.tgnx_link_predictor_bwd(0, 3, 4, 4, p, p, p, p, null, p, null, p, p, 1, p, p, p, null, p, null, p, p, p,
                                   1 << 20, null)
    assert rc != 0 and b"tgnx_link_predictor_bwd" in L.tgnx_last_error()
    need = L.tgnx_col_sum_ws_bytes(1000, 300)
    assert need >= 4 * 300 * 4                                # partials of ceil(1000 / 256) = 4 row chunks
    rc = L.tgnx_col_sum(1000, 300, p, 300, p, p, need - 1, null)
    assert rc != 0 and b"tgnx_col_sum" in L.tgnx_last_error() and b"workspace" in L.tgnx_last_error()
    rc = L.tgnx_col_sum(4, 8, p, 7, p, p, 1 << 20, null)      # ldx < N
    assert rc != 0 and b"tgnx_col_sum" in L.tgnx_last_error()
    assert keep.sum() == 0
