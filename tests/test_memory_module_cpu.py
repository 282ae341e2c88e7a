"""CPU checks of tgnx.nn.TGNMemory / DyRepMemory (tgb-tgn-dgl_amd/modules/memory_module.py re-exports them) and of the
device message store's entry points (csrc/tgnx_memstore.hip): constructing the modules and reading their state dicts
needs no GPU; names, order and shapes are those of oracle/tgn_ref.RefTGNMemory (itself pinned to the reference module
by tests/golden/tgn_memory_*.npz); the store tensors stay out of the state dict; the new torch ops are registered; the
new C entry points check their arguments before any device call."""
import ctypes

import numpy as np
import pytest
import torch


def _memory(aggr="last", cell="gru", cls=None, **kw):
    from tgnx import nn as T
    cls = cls or T.TGNMemory
    agg = T.LastAggregator() if aggr == "last" else T.MeanAggregator()
    return cls(40, 5, 8, 8, T.IdentityMessage(5, 8, 8), agg, cell, **kw)


@pytest.mark.parametrize("aggr", ["last", "mean"])
@pytest.mark.parametrize("cell", ["gru", "rnn"])
def test_state_dict_matches_oracle_and_loads_strict(aggr, cell):
    from oracle.tgn_ref import RefTGNMemory
    torch.manual_seed(0)
    ref = RefTGNMemory(40, 5, 8, 8, aggr=aggr, updater=cell)
    ref.memory.normal_()
    ref.last_update.random_(0, 1000)
    mine = _memory(aggr, cell)
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    mine.load_state_dict(b, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, b[k]), k


def test_dyrep_state_dict_matches_oracle():
    from oracle.tgn_ref import RefTGNMemory
    from tgnx import nn as T
    ref = RefTGNMemory(40, 5, 8, 8, aggr="last", updater="rnn", use_src_emb_in_msg=True)
    mine = _memory("last", "rnn", cls=T.DyRepMemory, use_src_emb_in_msg=True)
    assert mine.use_src_emb_in_msg and not mine.use_dst_emb_in_msg
    assert list(mine.state_dict().keys()) == list(ref.state_dict().keys())
    mine.load_state_dict(ref.state_dict(), strict=True)


def test_golden_parameter_set_loads(golden):
    z = golden("tgn_memory_last_gru.npz")
    N, d, D, B, n_train, n_eval = z["meta"].tolist()
    from tgnx import nn as T
    mine = T.TGNMemory(N, d, D, D, T.IdentityMessage(d, D, D), T.LastAggregator())
    sd = {k[2:].replace("__", "."): torch.from_numpy(z[k]) for k in z.files if k.startswith("p_")}
    assert sd
    res = mine.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"memory", "last_update", "_assoc"}
    for k, v in sd.items():
        assert torch.equal(mine.state_dict()[k], v), k


class _LinearMessage(torch.nn.Module):
    def __init__(self, in_dim, out_channels):
        super().__init__()
        self.out_channels = out_channels
        self.lin = torch.nn.Linear(in_dim, out_channels)

    def forward(self, z_src, z_dst, raw_msg, t_enc):
        return self.lin(torch.cat([z_src, z_dst, raw_msg, t_enc], dim=-1))


def test_submodules_and_updater_choice():
    from tgnx import nn as T
    msg = _LinearMessage(29, 11)
    mem = T.TGNMemory(40, 5, 8, 8, msg, T.LastAggregator())
    assert mem.msg_s_module is msg and mem.msg_d_module is not msg
    assert mem.msg_d_module.lin.weight is not msg.lin.weight
    assert torch.equal(mem.msg_d_module.lin.weight, msg.lin.weight)
    keys = list(mem.state_dict().keys())
    for k in ("msg_s_module.lin.weight", "msg_s_module.lin.bias", "msg_d_module.lin.weight", "msg_d_module.lin.bias"):
        assert k in keys, k
    assert isinstance(mem.time_enc, T.TimeEncoder) and isinstance(mem.memory_updater, T.MemoryCell)
    assert mem.memory_updater.input_size == 11 and mem.memory_updater.cell == "gru"
    assert mem.memory.shape == (40, 8) and mem.memory.dtype == torch.float32
    assert mem.last_update.shape == (40,) and mem.last_update.dtype == torch.long
    assert mem._assoc.shape == (40,) and mem._assoc.dtype == torch.long
    assert mem.device == mem.time_enc.lin.weight.device
    with pytest.raises(ValueError):
        T.TGNMemory(40, 5, 8, 8, T.IdentityMessage(5, 8, 8), T.LastAggregator(), "lstm")
    with pytest.raises(ValueError):
        T.DyRepMemory(40, 5, 8, 8, T.IdentityMessage(5, 8, 8), T.LastAggregator(), "lstm")


def test_store_tensors_are_buffers_outside_the_state_dict():
    mem = _memory(store_capacity=64)
    store = ("_log_src", "_log_dst", "_log_t", "_log_raw", "_arena", "_node_tab")
    bufs = dict(mem.named_buffers())
    sd = mem.state_dict()
    for k in store:
        assert k in bufs and k not in sd, k
    assert bufs["_log_src"].shape == (64,) and bufs["_log_raw"].shape == (64, 5) and bufs["_arena"].shape == (128,)
    assert bufs["_node_tab"].shape == (160,) and not bool(bufs["_node_tab"].any())
    mem.memory.fill_(1.0)
    mem.last_update.fill_(3)
    mem.reset_state()
    assert not bool(mem.memory.any()) and not bool(mem.last_update.any()) and mem._fill == 0


def test_memory_module_reexports():
    import modules
    import tgnx.nn as tnn
    from modules.memory_module import DyRepMemory, TGNMemory
    assert TGNMemory is tnn.TGNMemory and DyRepMemory is tnn.DyRepMemory
    assert modules.TGNMemory is tnn.TGNMemory and modules.DyRepMemory is tnn.DyRepMemory
    assert "TGNMemory" in tnn.__all__ and "DyRepMemory" in tnn.__all__


MEMSTORE_OPS = ("memstore_put", "memstore_count", "memstore_gather", "memstore_build_msg")


def test_memstore_ops_are_listed_and_registered():
    from tgnx import ops
    ns = ops.load()
    for name in MEMSTORE_OPS:
        assert name in ops.OPS, name
        assert hasattr(ns, name), name
    assert callable(ops.build_messages)


def _buf(n=256):
    a = np.zeros(n, dtype=np.int64)
    return a, ctypes.c_void_p(a.ctypes.data)


def _fails(L, rc, name, word=None):
    err = L.tgnx_last_error()
    assert rc != 0 and name in err, (rc, err)
    if word:
        assert word in err, err


def test_memstore_entry_points_check_arguments_before_any_device_call():
    """Each call fails in its argument check (host pointers are never touched; no HIP call is made)."""
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    # put(src, dst, t, raw, B, d, sorted, perm, start, cap, N, log_src, log_dst, log_t, log_raw, arena, tab, bad, s)
    put = L.tgnx_memstore_put
    _fails(L, put(null, p, p, p, 4, 5, p, p, 0, 64, 40, p, p, p, p, p, p, p, null), b"tgnx_memstore_put", b"null")
    _fails(L, put(p, p, p, p, 4, 5, p, p, 0, 64, 40, p, p, p, p, p, null, p, null), b"tgnx_memstore_put", b"null")
    _fails(L, put(p, p, p, p, -1, 5, p, p, 0, 64, 40, p, p, p, p, p, p, p, null), b"tgnx_memstore_put", b"sizes")
    _fails(L, put(p, p, p, p, 4, 5, p, p, 61, 64, 40, p, p, p, p, p, p, p, null), b"tgnx_memstore_put", b"capacity")
    # count(tab, N, n_id, M, put_bad, totals, ws, ws_bytes, s)
    need = L.tgnx_memstore_gather_ws_bytes(5000)
    assert need >= 2 * 5 * 8                                   # two offsets per tile of 1024 nodes
    cnt = L.tgnx_memstore_count
    _fails(L, cnt(p, 40, null, 7, null, p, p, 1 << 20, null), b"tgnx_memstore_count", b"null")
    _fails(L, cnt(p, 40, p, 7, null, null, p, 1 << 20, null), b"tgnx_memstore_count", b"null")
    _fails(L, cnt(p, 40, p, -7, null, p, p, 1 << 20, null), b"tgnx_memstore_count", b"sizes")
    _fails(L, cnt(p, 40, p, 5000, null, p, p, need - 1, null), b"tgnx_memstore_count", b"workspace")
    # gather(tab, N, arena, log_t, fill, n_id, M, n_s, n_d, slot, owner, t, lu, ws, ws_bytes, s)
    gat = L.tgnx_memstore_gather
    _fails(L, gat(p, 40, null, p, 9, p, 7, 3, 2, p, p, p, p, p, 1 << 20, null), b"tgnx_memstore_gather", b"null")
    _fails(L, gat(p, 40, p, p, 9, p, 7, 3, 2, p, p, p, null, p, 1 << 20, null), b"tgnx_memstore_gather", b"null")
    _fails(L, gat(p, 40, p, p, 9, p, 7, -3, 2, p, p, p, p, p, 1 << 20, null), b"tgnx_memstore_gather", b"sizes")
    _fails(L, gat(p, 40, p, p, 9, p, 5000, 3, 2, p, p, p, p, p, need - 1, null), b"tgnx_memstore_gather", b"workspace")
    # build(slot, n_msg, n_s, log_src, log_dst, log_t, log_raw, fill, N, D, d, T, memory, last_update, w, b, emb, E,
    #       assoc, stamp, n_id, M, emb_flags, out, t_rel, s)
    bld = L.tgnx_memstore_build_msg
    _fails(L, bld(p, 6, 3, p, p, p, p, 9, 40, 8, 5, 8, p, p, p, p, null, 0, null, null, null, 0, 0, null, p, null),
           b"tgnx_memstore_build_msg", b"null")
    _fails(L, bld(p, 6, 3, p, p, p, p, 9, 40, 8, 5, 8, null, p, p, p, null, 0, null, null, null, 0, 0, p, p, null),
           b"tgnx_memstore_build_msg", b"null")
    _fails(L, bld(p, -6, 0, p, p, p, p, 9, 40, 8, 5, 8, p, p, p, p, null, 0, null, null, null, 0, 0, p, p, null),
           b"tgnx_memstore_build_msg", b"sizes")
    _fails(L, bld(p, 6, 7, p, p, p, p, 9, 40, 8, 5, 8, p, p, p, p, null, 0, null, null, null, 0, 0, p, p, null),
           b"tgnx_memstore_build_msg", b"sizes")
    # embeddings without the membership inputs
    _fails(L, bld(p, 6, 3, p, p, p, p, 9, 40, 8, 5, 8, p, p, p, p, p, 4, null, null, null, 0, 1, p, p, null),
           b"tgnx_memstore_build_msg", b"assoc")
    assert keep.sum() == 0
