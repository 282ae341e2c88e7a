"""The TGN memory path (SURVEY §8 a14–a16) behind the reference's PyG surface.

`getModel` / `getOptimizer` mirror pyg_model_utils.py:10-43: the returned dict has 'memory' (TGNMemory:
time_enc + GRUCell, memory / last_update buffers, message stores), 'gnn' (GraphAttentionEmbedding:
TransformerConv, sharing memory.time_enc) and 'link_pred' (LinkPredictor); state_dict keys are the
reference's (`memory.memory_updater.weight_ih`, `gnn.conv.lin_key.weight`, `link_pred.lin_final.bias`, ...).  Every
trainable tensor is a view into one flat fp32 device buffer (`tgnx_tgn_param_layout`); the step runs in
libtgnx (TgnEngine below), there is no torch-op path.

Initialisation as the reference's modules: TimeEncoder = Linear(1, D) (torch default), GRUCell
U(-1/sqrt(D), 1/sqrt(D)), PyG Linear (kaiming_uniform a=sqrt(5) -> U(-1/sqrt(in), 1/sqrt(in)), bias the
same bound), LinkPredictor torch Linear defaults; memory / last_update zero (memory_module.py:106-110).
"""
from __future__ import annotations

import ctypes
import os
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib

P = ctypes.c_void_p

PARAM_ORDER = [  # flat-buffer order = tgnx_tgn_param_layout
    "memory.time_enc.lin.weight", "memory.time_enc.lin.bias",
    "memory.memory_updater.weight_ih", "memory.memory_updater.weight_hh", "memory.memory_updater.bias_ih",
    "memory.memory_updater.bias_hh",
    "gnn.conv.lin_key.weight", "gnn.conv.lin_key.bias", "gnn.conv.lin_query.weight", "gnn.conv.lin_query.bias",
    "gnn.conv.lin_value.weight", "gnn.conv.lin_value.bias", "gnn.conv.lin_edge.weight",
    "gnn.conv.lin_skip.weight", "gnn.conv.lin_skip.bias",
    "link_pred.lin_src.weight", "link_pred.lin_src.bias", "link_pred.lin_dst.weight", "link_pred.lin_dst.bias",
    "link_pred.lin_final.weight", "link_pred.lin_final.bias",
]
# layers = 2 (2-hop temporal attention, SURVEY §8d comment config): gnn.conv2 after the 21 above
PARAM_ORDER2 = PARAM_ORDER + [
    "gnn.conv2.lin_key.weight", "gnn.conv2.lin_key.bias", "gnn.conv2.lin_query.weight", "gnn.conv2.lin_query.bias",
    "gnn.conv2.lin_value.weight", "gnn.conv2.lin_value.bias", "gnn.conv2.lin_edge.weight",
    "gnn.conv2.lin_skip.weight", "gnn.conv2.lin_skip.bias",
]


class TgnConfig(ctypes.Structure):
    _fields_ = [("num_nodes", ctypes.c_int64), ("num_events", ctypes.c_int64), ("ring", ctypes.c_int32),
                ("mem_dim", ctypes.c_int32), ("msg_dim", ctypes.c_int32), ("heads", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("max_neg", ctypes.c_int32), ("aggr", ctypes.c_int32),
                ("dropout", ctypes.c_float), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("layers", ctypes.c_int32),
                ("updater", ctypes.c_int32), ("emb_in_msg", ctypes.c_int32)]


class TgnBuffers(ctypes.Structure):
    _fields_ = [("ev_src", P), ("ev_dst", P), ("ev_t", P), ("ev_msg", P), ("neg", P), ("dst_nodes", P),
                ("n_dst", ctypes.c_int64), ("nbr", P), ("eid", P), ("rt", P), ("assoc", P), ("memory", P),
                ("last_update", P), ("store", P), ("node_gen", P), ("params", P), ("grads", P), ("adam_m", P),
                ("adam_v", P), ("ctl", P), ("out_pos", P), ("out_neg", P), ("mrr", P), ("ws", P), ("xrows", P),
                ("xcap", ctypes.c_int64), ("out_ev", P), ("plan_table", P), ("flags", ctypes.c_int32)]


class TgnGrowOut(ctypes.Structure):      # tgnx_tgn_grow_out: the new allocations of tgnx_tgn_grow_nodes
    _fields_ = [("nbr", P), ("eid", P), ("rt", P), ("assoc", P), ("memory", P), ("last_update", P), ("node_gen", P),
                ("store", P)]


# the memory modules' updater cell: TGNMemory.memory_updater (memory_module.py:70-78, memory_updater_cell
# 'gru' | 'rnn') and DyRepMemory.memory_updater (:259-264, memory_updater_type) — the same state-dict names
MEMORY_TYPES = ("tgn", "dyrep")


def param_shapes(D: int, d: int, layers: int = 1, updater: str = "gru") -> dict:
    Q = 3 * D + d
    G3 = 1 if updater == "rnn" else 3     # RNNCell: [D, .]; GRUCell: [3D, .] (r, z, n)
    u = "memory.memory_updater"
    s = {"memory.time_enc.lin.weight": (D, 1), "memory.time_enc.lin.bias": (D,),
         f"{u}.weight_ih": (G3 * D, Q), f"{u}.weight_hh": (G3 * D, D),
         f"{u}.bias_ih": (G3 * D,), f"{u}.bias_hh": (G3 * D,),
         "gnn.conv.lin_edge.weight": (D, D + d),
         "link_pred.lin_src.weight": (D, D), "link_pred.lin_src.bias": (D,),
         "link_pred.lin_dst.weight": (D, D), "link_pred.lin_dst.bias": (D,),
         "link_pred.lin_final.weight": (1, D), "link_pred.lin_final.bias": (1,)}
    convs = ("conv", "conv2") if layers == 2 else ("conv",)
    for cv in convs:
        for k in ("key", "query", "value", "skip"):
            s[f"gnn.{cv}.lin_{k}.weight"] = (D, D)
            s[f"gnn.{cv}.lin_{k}.bias"] = (D,)
        s[f"gnn.{cv}.lin_edge.weight"] = (D, D + d)
    return s


def reference_init(D: int, d: int, generator=None, layers: int = 1, updater: str = "gru") -> dict:
    g = generator

    def unif(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    out = {}
    for name, shape in param_shapes(D, d, layers, updater).items():
        if name.startswith("memory.time_enc"):
            bound = 1.0                                   # Linear(1, D): fan_in = 1
        elif name.startswith("memory.memory_updater"):
            bound = 1.0 / math.sqrt(D)                    # GRUCell / RNNCell.reset_parameters
        elif name.endswith("lin_edge.weight"):
            bound = 1.0 / math.sqrt(D + d)
        else:
            bound = 1.0 / math.sqrt(D)                    # fan_in D (conv / predictor linears)
        out[name] = unif(shape, bound)
    return out


class _Holder(nn.Module):
    pass


class TGNModel(nn.Module):
    """memory + gnn + link_pred of pyg_model_utils.py:10-36 over one flat parameter buffer.

    memory = "tgn": TGNMemory (modules/memory_module.py:25-215) with memory_updater_cell = updater,
    "gru" (GRUCell, the default) or "rnn" (RNNCell, :70-78);
    memory = "dyrep": DyRepMemory (modules/memory_module.py:218-421) with memory_updater_type = updater; its
    use_src_emb_in_msg / use_dst_emb_in_msg (:387-408) build update_state's messages with the batch's
    embeddings (the TransformerConv output of the same forward: train / eval) in place of the memory rows of
    endpoints in src ∪ dst (1-hop embedding, world 1).  Without them its update order, messages and
    state-dict names are TGNMemory's."""

    def __init__(self, num_nodes, num_events, msg_dim, hidden_dim, device, ring=10, max_batch=2048, max_neg=1,
                 aggr="last", dropout=0.1, generator=None, layers=1, memory="tgn", updater="gru",
                 use_src_emb_in_msg=False, use_dst_emb_in_msg=False):
        super().__init__()
        if memory not in MEMORY_TYPES:
            raise ValueError(f"memory must be 'tgn' or 'dyrep', got {memory!r}")
        if updater not in ("gru", "rnn"):
            raise ValueError(f"Memory updater can be either 'gru' or 'rnn' (memory_module.py:75-78), got {updater!r}")
        emb = (1 if use_src_emb_in_msg else 0) | (2 if use_dst_emb_in_msg else 0)
        if emb and memory != "dyrep":
            raise ValueError("use_src/dst_emb_in_msg are DyRepMemory options (memory='dyrep'; memory_module.py:242-245)")
        if emb and int(layers) != 1:
            raise NotImplementedError("DyRep embedding messages are built for the 1-hop embedding (layers = 1)")
        self.memory_type, self.updater = memory, updater
        dev = _lib.require_device(device)
        D, d = int(hidden_dim), int(msg_dim)
        num_events = max(int(num_events or 0), 1)
        self.num_nodes, self.num_events, self.D, self.d = int(num_nodes), num_events, D, d
        self.cfg = TgnConfig(num_nodes=num_nodes, num_events=num_events, ring=ring, mem_dim=D, msg_dim=d, heads=2,
                             max_batch=max_batch, max_neg=max_neg, aggr=0 if aggr == "last" else 1, dropout=dropout,
                             lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, layers=int(layers),
                             updater=1 if updater == "rnn" else 0, emb_in_msg=emb)
        if layers not in (1, 2):
            raise ValueError(f"layers must be 1 or 2, got {layers}")
        self.layers = int(layers)
        order = PARAM_ORDER2 if layers == 2 else PARAM_ORDER
        self.param_order = order
        off = (ctypes.c_int64 * (len(order) + 1))()
        _lib.call("tgnx_tgn_param_layout", ctypes.byref(self.cfg), off)
        self.offsets = list(off)
        total = self.offsets[-1]
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad_flat = torch.zeros(total + 1, dtype=torch.float32, device=dev)    # + batch-loss slot
        shapes = param_shapes(D, d, layers, updater)
        init = reference_init(D, d, generator, layers, updater)
        self.memory = _Holder()
        self.memory.time_enc = _Holder()
        self.memory.time_enc.lin = _Holder()
        self.memory.memory_updater = _Holder()
        self.gnn = _Holder()
        self.gnn.conv = _Holder()
        if layers == 2:
            self.gnn.conv2 = _Holder()
        for cv in (("conv", "conv2") if layers == 2 else ("conv",)):
            for k in ("key", "query", "value", "edge", "skip"):
                setattr(getattr(self.gnn, cv), f"lin_{k}", _Holder())
        self.link_pred = _Holder()
        for k in ("src", "dst", "final"):
            setattr(self.link_pred, f"lin_{k}", _Holder())
        self._views = {}
        for name, o in zip(order, self.offsets[:-1]):
            n = int(np.prod(shapes[name]))
            view = self.flat[o:o + n].view(shapes[name])
            view.copy_(init[name].to(dev))
            mod = self
            parts = name.split(".")
            for part in parts[:-1]:
                mod = getattr(mod, part)
            setattr(mod, parts[-1], nn.Parameter(view))
            self._views[name] = (o, n, shapes[name])
        self.gnn.time_enc = self.memory.time_enc                           # shared (pyg_model_utils.py:27)
        # TGNMemory buffers (memory_module.py:80-83) and the message stores
        self.memory.register_buffer("memory", torch.zeros(num_nodes, D, device=dev))
        self.memory.register_buffer("last_update", torch.zeros(num_nodes, dtype=torch.long, device=dev))
        self.store = None
        self.ensure_events(max(int(num_events or 0), 1))
        self.node_gen = torch.zeros(num_nodes, dtype=torch.int32, device=dev)
        # bumped by every parameter load: an engine's embedding table compares it at refresh
        self._param_version = 0

    def ensure_events(self, n: int) -> None:
        """Size the message-store arena for an event table of n rows (the reference's getModel does
        not know the stream length; the engine calls this when it binds the table)."""
        if self.store is not None and n <= self.cfg.num_events:
            return
        self.cfg.num_events = int(n)
        self.num_events = int(n)
        words = _lib.lib().tgnx_tgn_store_words(ctypes.byref(self.cfg))
        if words == 0:
            raise RuntimeError(f"tgnx_tgn_store_words: {_lib.lib().tgnx_last_error().decode()}")
        old = self.store
        self.store = torch.zeros(int(words), dtype=torch.long, device=self.flat.device)
        if old is not None:   # per-node {off, cnt} words first; arena offsets stay valid
            self.store[:old.numel()].copy_(old)

    @property
    def node_capacity(self) -> int:
        """Rows of the allocations under memory / last_update / node_gen (they are the first num_nodes rows once the
        node space has grown)."""
        alloc = getattr(self, "_node_alloc", None)
        return self.num_nodes if alloc is None else int(alloc[0].shape[0])

    def _install_nodes(self, memory, last_update, node_gen, store, num_nodes: int) -> None:
        """Take allocations of >= num_nodes rows whose first rows hold the state, and the store laid out for
        num_nodes: the memory / last_update buffers are registered again as their first num_nodes rows (contiguous
        views: state_dict() keeps the reference's names and [N, .] shapes), cfg.num_nodes follows."""
        n = int(num_nodes)
        self._node_alloc = (memory, last_update, node_gen)
        self.memory.register_buffer("memory", memory[:n])
        self.memory.register_buffer("last_update", last_update[:n])
        self.node_gen = node_gen[:n]
        self.store = store
        self.cfg.num_nodes = n
        self.num_nodes = n

    def grow_nodes(self, n: int) -> int:
        """Extend the node space to n nodes in place (n <= num_nodes: a no-op); returns num_nodes afterwards.  Rows
        [0, N) of memory, last_update, node_gen and the stores are unchanged bit for bit, the new rows are what
        reset_state leaves (zeros, empty store runs); no parameter moves.  With an engine bound the call goes through
        it (TgnEngine.grow_nodes: the ring, the workspace and the bindings follow); a model on its own moves only its
        own tensors (tgnx_tgn_grow_nodes) and its loader must be grown too (LastNeighborLoader.grow) before an engine
        binds the pair."""
        f = self._tgnx_grow() if getattr(self, "_tgnx_grow", None) is not None else None
        if f is not None:
            return f(n)
        n, N = int(n), self.num_nodes
        if not check_grow_args(N, n):
            return N
        dev = self.flat.device
        torch.cuda.synchronize(dev)
        rows = n > self.node_capacity
        old = dict(memory=self.memory.memory, last_update=self.memory.last_update, node_gen=self.node_gen,
                   store=self.store)
        new = grow_node_tensors(dev, N, n, n, self.cfg.ring, self.D, self.cfg.num_events, old, rows=rows)
        alloc = (new["memory"], new["last_update"], new["node_gen"]) if rows else self._node_alloc
        self._install_nodes(*alloc, new["store"], n)
        return n

    @property
    def device(self):
        return self.flat.device

    def trainable_count(self) -> int:
        return sum(n for _, n, _ in self._views.values())

    def load_reference_state(self, sd: dict) -> None:
        with torch.no_grad():
            for name, (o, n, _) in self._views.items():
                self.flat[o:o + n].copy_(sd[name].reshape(-1).to(self.flat.device))
        self._param_version += 1

    def grads_by_name(self) -> dict:
        """The last step's gradient of every parameter tensor (views into grad_flat).  Raises while an engine runs
        this model's steps with keep_grads=False (bench.py, the drop-in train()): those fused steps do not store the
        gradient (TGNX_TGN_NO_GRAD_STORE), so grad_flat would hold a stale step's values."""
        if getattr(self, "_grads_stale", False):
            raise RuntimeError("grads_by_name: the bound TgnEngine runs with keep_grads=False (fused Adam without the "
                               "gradient store): set engine.keep_grads = True before binding to read gradients")
        return {name: self.grad_flat[o:o + n].view(s) for name, (o, n, s) in self._views.items()}

    def settle(self) -> None:
        """Apply a data-parallel engine's deferred exchange (TgnEngine.finish) so that memory, last_update,
        the parameters and the Adam moments are current.  state_dict() calls it; direct
        reads of model.flat / model.memory.* between data-parallel steps need it (or engine.finish())."""
        f = self._tgnx_finish() if getattr(self, "_tgnx_finish", None) is not None else None
        if f is not None:
            f()
        self.invalidate_prefetch()   # (the caller may go on to write the tensors it reads: state_dict() returns the buffers)

    def invalidate_prefetch(self) -> None:
        """Tell the bound engine that memory / last_update / the stores may have been rewritten behind it: its next
        resident step prepares its batch again instead of using what the previous step gathered ahead
        (TgnEngine.gather_ahead)."""
        f = self._tgnx_invalidate() if getattr(self, "_tgnx_invalidate", None) is not None else None
        if f is not None:
            f()

    def state_dict(self, *a, **k):
        self.settle()
        return super().state_dict(*a, **k)

    def load_state_dict(self, *a, **k):
        self.settle()
        out = super().load_state_dict(*a, **k)
        self.invalidate_prefetch()
        self._param_version += 1
        return out

    def forward(self, *a, **k):
        raise RuntimeError("tgnx TGN runs through tgnx.tgn.TgnEngine / pyg_epoch_utils (the fused HIP step)")


class TgnAdam(torch.optim.Optimizer):
    """torch.optim.Adam over set(memory) | set(gnn) | set(link_pred) (pyg_model_utils.py:38-43); the
    update runs on the device (tgnx_tgn_train_update)."""

    def __init__(self, model: TGNModel, lr: float):
        super().__init__([p for p in model.parameters() if p.requires_grad], dict(lr=lr, betas=(0.9, 0.999), eps=1e-8))
        self.model = model
        model.cfg.lr = float(lr)
        self.exp_avg = torch.zeros_like(model.flat)
        self.exp_avg_sq = torch.zeros_like(model.flat)

    def zero_grad(self, set_to_none: bool = True):
        pass

    def step(self, closure=None):
        raise RuntimeError("TgnAdam.step runs inside the TGN train step (tgnx_tgn_train_update)")


def row_header(v: int, lu: int) -> list:
    """Header of an exchanged memory row (include/tgnx.h TGNX_TGN_ROW; written on the device by the
    update step): node, last_update bits 0-23 / 24-47 / 48-63, each a float holding an exact integer."""
    b = int(lu) & 0xFFFFFFFFFFFFFFFF
    return [float(v), float(b & 0xFFFFFF), float((b >> 24) & 0xFFFFFF), float(b >> 48)]


def row_decode(h) -> tuple:
    """(node, last_update) of an exchanged row header (node -1: unused slot)."""
    b = int(h[1]) | (int(h[2]) << 24) | (int(h[3]) << 48)
    return int(h[0]), b - (1 << 64) if b >= 1 << 63 else b


def _p(t):
    return 0 if t is None else t.data_ptr()


def grown_capacity(cap: int, need: int) -> int:
    """Row capacity of the event table for `need` rows when it holds `cap`: unchanged while they fit, else the larger
    of `need` and 1.5 x cap — geometric, so n appended rows cost O(n) copied rows in all."""
    cap, need = int(cap), int(need)
    if cap < 0 or need < 0:
        raise ValueError(f"grown_capacity: negative row count ({cap}, {need})")
    return cap if need <= cap else max(need, cap + cap // 2)


def grown_node_capacity(cap: int, need: int) -> int:
    """Row capacity of the node tensors for `need` nodes when they hold `cap`: unchanged while they fit, else the
    larger of `need` and 1.25 x cap — geometric, so n nodes added one at a time cost O(n) copied rows in all (about
    5 n).  The factor is below the event table's 1.5: a node row (memory, three ring rows, five words) is several
    times an event row, and capacity rows are allocated, initialised and never read."""
    cap, need = int(cap), int(need)
    if cap < 0 or need < 0:
        raise ValueError(f"grown_node_capacity: negative node count ({cap}, {need})")
    return cap if need <= cap else max(need, cap + cap // 4)


MAX_NODES = 1 << 31    # node ids cross the C ABI checks as values below 2^31 (include/tgnx.h)


def check_grow_args(num_nodes: int, n: int, world: int = 1, dp: bool = False) -> bool:
    """Whether grow_nodes(n) has anything to do (n > num_nodes), or ValueError: one device, n below 2^31."""
    if world > 1 or dp:
        raise ValueError("grow_nodes: one device only (world > 1 / the data-parallel step forms are not built)")
    n = int(n)
    if n >= MAX_NODES:
        raise ValueError(f"grow_nodes: {n} nodes; node ids are below 2^31")
    return n > int(num_nodes)


def check_append_args(validate: bool, grow: bool) -> None:
    """ValueError for append_events(validate=False, grow=True): growing needs the host read validation makes."""
    if grow and not validate:
        raise ValueError("append_events: grow=True needs validate=True (the node space is sized from the one host "
                         "read of the ids that validation makes)")


# name in tgnx_tgn_buffers / tgnx_tgn_grow_out -> (trailing shape from (ring, mem_dim), dtype) of a [N, .] tensor
NODE_ROW_TENSORS = {
    "nbr": (lambda K, D: (K,), torch.long), "eid": (lambda K, D: (K,), torch.long),
    "rt": (lambda K, D: (K,), torch.float32), "assoc": (lambda K, D: (), torch.long),
    "memory": (lambda K, D: (D,), torch.float32), "last_update": (lambda K, D: (), torch.long),
    "node_gen": (lambda K, D: (), torch.int32),
}


def grow_node_tensors(dev, N: int, n_new: int, cap: int, ring: int, mem_dim: int, num_events: int, old: dict,
                      rows: bool = True) -> dict:
    """tgnx_tgn_grow_nodes over the tensors in `old` (keys of NODE_ROW_TENSORS, each [N, .], and 'store'): returns
    the new allocations by the same keys — row tensors of `cap` rows (rows [N, cap) as reset_state leaves them), the
    store re-laid for n_new nodes over an arena of 2 * num_events words — after one host read of the device's count
    of store runs outside the arena: RuntimeError if there is one, and the caller still holds the old tensors.
    rows=False re-lays the store alone (tgnx_tgn_grow_store: growth inside the row capacity)."""
    N, n_new, cap, K, D, nev = int(N), int(n_new), int(cap), int(ring), int(mem_dim), max(int(num_events), 1)
    cfg = TgnConfig(num_nodes=N, num_events=nev, ring=K, mem_dim=D)
    b, out, new = TgnBuffers(), TgnGrowOut(), {}
    for k, (shape, dt) in NODE_ROW_TENSORS.items():
        x = old.get(k)
        if x is None or not rows:
            continue
        if tuple(x.shape) != (N,) + shape(K, D) or x.dtype != dt or not x.is_contiguous():
            raise ValueError(f"grow_nodes: {k} is {tuple(x.shape)} {x.dtype}, expected contiguous "
                             f"{(N,) + shape(K, D)} {dt}")
        new[k] = torch.zeros((cap,) + shape(K, D), dtype=dt, device=dev)
        setattr(b, k, x.data_ptr())
        setattr(out, k, new[k].data_ptr())
    st = old.get("store")
    if st is not None and n_new > N:
        if st.dtype != torch.long or st.numel() < 4 * N + 2 * nev or not st.is_contiguous():
            raise ValueError(f"grow_nodes: the store holds {st.numel()} words, 4 * {N} + 2 * {nev} expected")
        new["store"] = torch.zeros(4 * n_new + 2 * nev, dtype=torch.long, device=dev)
        b.store, out.store = st.data_ptr(), new["store"].data_ptr()
    if not new:
        return new
    bad = torch.zeros(1, dtype=torch.long, device=dev)
    if rows:
        _lib.call("tgnx_tgn_grow_nodes", ctypes.byref(cfg), ctypes.byref(b), n_new, cap, ctypes.byref(out), _p(bad),
                  _lib.stream(dev))
    else:
        _lib.call("tgnx_tgn_grow_store", ctypes.byref(cfg), ctypes.byref(b), n_new, _p(new["store"]), _p(bad),
                  _lib.stream(dev))
    n_bad = int(bad.item())
    if n_bad:
        raise RuntimeError(f"grow_nodes: {n_bad} message-store runs outside the arena's {2 * nev} words; nothing was "
                           "changed")
    return new


def check_event_rows(n_src: int, n_dst: int, n_t: int, msg_shape: tuple, msg_dim: int) -> int:
    """The row count of an appended chunk, or ValueError: src, dst, t of one length n and msg [n, msg_dim]."""
    n = int(n_src)
    if int(n_dst) != n or int(n_t) != n:
        raise ValueError(f"append_events: src, dst, t must have one length, got {n_src}, {n_dst}, {n_t}")
    if len(msg_shape) != 2 or tuple(int(x) for x in msg_shape) != (n, int(msg_dim)):
        raise ValueError(f"append_events: msg must be [n, msg_dim] = [{n}, {msg_dim}], got {tuple(msg_shape)}")
    return n


def check_observe_args(start: int, B: int, max_batch: int, num_events: int, world: int = 1) -> None:
    """ValueError unless rows [start, start + B) are a batch observe() can take: 0 <= B <= max_batch, inside the
    table's valid rows, one device."""
    if world > 1:
        raise ValueError("observe: one device only (world > 1 is not built)")
    if B < 0 or B > max_batch:
        raise ValueError(f"observe: B = {B} outside [0, max_batch = {max_batch}]")
    if start < 0 or start + B > num_events:
        raise ValueError(f"observe: rows [{start}, {start + B}) outside the event table ({num_events} events)")


EXPLAIN_MODES = {"slot": 0, "neighbour": 1}      # TGNX_EXPLAIN_SLOT / TGNX_EXPLAIN_NEIGHBOUR


def check_explain_args(by, n_src: int, n_dst: int, layers: int = 1, world: int = 1) -> int:
    """explain()'s arguments: the removal set's name, one destination per source, a 1-hop engine on one device.
    Returns the C ABI's mode code."""
    if by not in EXPLAIN_MODES:
        raise ValueError(f"explain: by must be one of {sorted(EXPLAIN_MODES)}, got {by!r}")
    if n_src != n_dst:
        raise ValueError(f"explain: {n_src} sources for {n_dst} destinations")
    if layers == 2:
        raise NotImplementedError("explain: leave-one-out effects are built for the 1-hop embedding (layers = 1): at 2 "
                                  "hops removing an edge also changes the node's own hop-1 row; attention() works")
    if world > 1:
        raise NotImplementedError("explain: one device only (world > 1: a data-parallel engine)")
    return EXPLAIN_MODES[by]


def check_compact_args(num_events: int, upto=None, capacity=None, world: int = 1) -> int:
    """The resolved `upto` of compact_events (default num_events), or ValueError: one device, 0 <= upto <= num_events,
    capacity (when given) at least 1."""
    if world > 1:
        raise ValueError("compact_events: one device only (world > 1 is not built)")
    num_events = int(num_events)
    upto = num_events if upto is None else int(upto)
    if upto < 0 or upto > num_events:
        raise ValueError(f"compact_events: upto = {upto} outside [0, num_events = {num_events}]")
    if capacity is not None and int(capacity) < 1:
        raise ValueError(f"compact_events: capacity = {capacity} must be at least 1")
    return upto


def check_forget_args(num_nodes: int, n_ids: int, world: int = 1, dp: bool = False) -> bool:
    """Whether forget_nodes has anything to do (n_ids > 0), or ValueError: one device, a node space to forget from,
    fewer than 2^31 ids (duplicates are allowed, so the list may be longer than num_nodes)."""
    if world > 1 or dp:
        raise ValueError("forget_nodes: one device only (world > 1 / the data-parallel step forms are not built)")
    num_nodes, n_ids = int(num_nodes), int(n_ids)
    if num_nodes < 1:
        raise ValueError(f"forget_nodes: num_nodes = {num_nodes}")
    if n_ids < 0 or n_ids >= MAX_NODES:
        raise ValueError(f"forget_nodes: {n_ids} ids; an id list holds fewer than 2^31")
    return n_ids > 0


FORGET_COUNTS = ("nodes", "ring_slots", "ring_rows", "store_entries")    # record words 0..3 of tgnx_tgn_forget_plan


def compact_capacity(n_live: int, capacity=None) -> int:
    """Row capacity of the compacted table: `capacity` when given (ValueError below n_live), else what grown_capacity
    gives a full table of n_live rows for one more row — max(n_live + 1, 1.5 x n_live) — so that the next append does
    not reallocate at once."""
    n_live = int(n_live)
    if n_live < 0:
        raise ValueError(f"compact_events: negative live row count {n_live}")
    if capacity is not None:
        if int(capacity) < max(n_live, 1):
            raise ValueError(f"compact_events: capacity = {capacity} below the {n_live} live rows")
        return int(capacity)
    return grown_capacity(n_live, n_live + 1)


STREAM_STATE_FORMAT = 1
STREAM_FINGERPRINT = ("num_nodes", "ring", "mem_dim", "msg_dim")
# key -> shape in terms of (N, K, D, d, n = num_events); the ints of the dict are format, the fingerprint, num_events
STREAM_STATE_TENSORS = {
    "src": lambda N, K, D, d, n: (n,), "dst": lambda N, K, D, d, n: (n,), "t": lambda N, K, D, d, n: (n,),
    "msg": lambda N, K, D, d, n: (n, d),
    "memory": lambda N, K, D, d, n: (N, D), "last_update": lambda N, K, D, d, n: (N,),
    "node_gen": lambda N, K, D, d, n: (N,),
    "store_nodes": lambda N, K, D, d, n: (N, 4), "store_arena": lambda N, K, D, d, n: (2 * n,),
    "neighbors": lambda N, K, D, d, n: (N, K), "e_id": lambda N, K, D, d, n: (N, K), "ring_t": lambda N, K, D, d, n: (N, K),
    "ctl": lambda N, K, D, d, n: (24,),
}
STREAM_STATE_KEYS = ("format",) + STREAM_FINGERPRINT + ("num_events",) + tuple(STREAM_STATE_TENSORS)


def stream_fingerprint(cfg) -> dict:
    """What a stream state must share with the engine that loads it."""
    return {k: int(getattr(cfg, k)) for k in STREAM_FINGERPRINT}


def check_stream_state(state, fingerprint: dict) -> int:
    """num_events of a stream_state() dict, or ValueError: format 1, the engine's fingerprint, every key present and
    every tensor of the shape the ints imply.  Reads shapes only (no tensor contents, nothing on a device)."""
    if not isinstance(state, dict) or "format" not in state:
        raise ValueError("load_stream_state: not a stream_state() dict (no 'format')")
    if state["format"] != STREAM_STATE_FORMAT:
        raise ValueError(f"load_stream_state: format {state['format']!r}, this build reads {STREAM_STATE_FORMAT}")
    missing = [k for k in STREAM_STATE_KEYS if k not in state]
    if missing:
        raise ValueError(f"load_stream_state: missing keys {missing}")
    got = {k: int(state[k]) for k in STREAM_FINGERPRINT}
    if got != {k: int(fingerprint[k]) for k in STREAM_FINGERPRINT}:
        raise ValueError(f"load_stream_state: the state's fingerprint {got} is not the engine's {dict(fingerprint)}")
    n = int(state["num_events"])
    if n < 0:
        raise ValueError(f"load_stream_state: num_events = {n}")
    dims = (got["num_nodes"], got["ring"], got["mem_dim"], got["msg_dim"], n)
    for k, shape in STREAM_STATE_TENSORS.items():
        have = tuple(int(x) for x in getattr(state[k], "shape", (-1,)))
        if have != tuple(shape(*dims)):
            raise ValueError(f"load_stream_state: {k} has shape {have}, expected {tuple(shape(*dims))}")
    return n


def check_stream_state_grow(state, fingerprint: dict) -> tuple:
    """check_stream_state for load_stream_state(grow=True): (num_events, the state's num_nodes), or ValueError.  The
    state's num_nodes may differ from the engine's (>= 1, below 2^31) — more: the engine grows first, fewer: the rows
    beyond are reset rows — and nothing else is relaxed: format, keys, ring / mem_dim / msg_dim and every shape, the
    [N, .] ones by the state's own num_nodes."""
    if not isinstance(state, dict) or "num_nodes" not in state:
        return check_stream_state(state, fingerprint), int(fingerprint["num_nodes"])   # (raises: format / keys)
    ns = int(state["num_nodes"])
    if ns < 1 or ns >= MAX_NODES:
        raise ValueError(f"load_stream_state: num_nodes = {ns}")
    fp = dict(fingerprint)
    fp["num_nodes"] = ns
    return check_stream_state(state, fp), ns


EXCHANGE_MODES = ("fused", "split")


def exchange_collectives(comm, G: int, rank: int, world: int, mode: str = "fused", async_op: bool = False):
    """The data-parallel step's exchange over comm = [G gradient floats | world row slots] (each rank's kernels
    wrote its own slot):
      fused — ONE all-reduce of the whole buffer: the gradient sum, and (the other slots holding zeros) the
              all-gather of the rows, bit-exact (TgnEngine.__init__);
      split — an all-reduce of the G gradient floats and an in-place all_gather_into_tensor of the row slots:
              two collectives, but the rows travel once instead of as W-times-padded zeros in a sum.
    Returns the work handles (async_op) or []."""
    import torch.distributed as dist
    if mode == "split":
        rows = comm[G:]
        n = rows.numel() // world
        w1 = dist.all_reduce(comm[:G], async_op=async_op)
        w2 = dist.all_gather_into_tensor(rows, rows[rank * n:(rank + 1) * n], async_op=async_op)
        return [w for w in (w1, w2) if w is not None]
    if mode != "fused":
        raise ValueError(f"exchange mode must be one of {EXCHANGE_MODES}, got {mode!r}")
    w = dist.all_reduce(comm, async_op=async_op)
    return [] if w is None else [w]


class TgnEngine:
    """Owns the workspace of one TGN model + one neighbour ring over a resident event table
    (src, dst, t, msg rows = e_id).

    Data parallel (world > 1) resident steps defer the exchanged memory rows and Adam of step k to the head of
    step k + 1 (tgnx_tgn_train_fwd_bwd_pp).  Between such steps memory, last_update, the parameters and the
    Adam moments are one apply behind: call finish() before reading them directly.  check(), loss_sum(),
    flush(), eval / reset / binding calls and model.state_dict() do so themselves (the gradient buffer is final
    once the step's exchange returned: the apply does not change it).

    Gather-ahead (gather_ahead, default on; world-1 parity-set steps at 1 hop with LastAggregator, the GRU cell and
    TGNMemory messages): a prefetched step also copies the NEXT batch's message rows out of memory / last_update /
    the stores, inside its last launch.  Every other engine call, a loader version change, model.load_state_dict(),
    model.settle() / state_dict() and model.invalidate_prefetch() make the next step prepare its batch again.  A raw
    tensor write to memory / last_update / the stores between two resident steps without one of these is seen by the
    GRU's hidden-state operand but not by the pre-gathered message rows: call invalidate_prefetch() after it.

    A long-running stream (world 1): compact_events() retires the event rows that neither the ring nor a message
    store references and renumbers the rest in order, so the device footprint follows the live rows instead of the
    stream's length; stream_state() / load_stream_state() checkpoint the table, memory, stores, ring and ctl.  Both
    drop the resident bindings, the plan table and the captured graphs: bind again in the new numbering.

    Nodes that first appear after the model was built (world 1): grow_nodes(n) / observe_events(..., grow=True) extend
    the node space in place — memory, last_update, node_gen, the ring, the stores and the workspace move into larger
    allocations (tgnx_tgn_grow_nodes), old rows bit for bit, new rows as reset_state leaves them — and cfg.num_nodes
    stays the logical count over a row capacity (node_capacity, reserve_nodes).  Captured graphs are dropped, the
    resident bindings are made again.

    Nodes that leave (world 1): forget_nodes(ids) makes a node's memory, stores and ring row a never-seen node's and
    removes every other node's ring slots and stored messages that name it, in place (tgnx_tgn_forget_plan / _apply);
    what its past messages did to its partners' memory stays.  Bindings and graphs are dropped as a compaction drops
    them."""

    def __init__(self, model: TGNModel, loader, events: dict, optimizer: TgnAdam | None = None,
                 dst_nodes=None, seed: int = 0, rank: int = 0, world: int = 1, data_parallel: bool | None = None):
        self.model, self.loader, self.opt = model, loader, optimizer
        self.dev = model.device
        import weakref
        model._tgnx_finish = weakref.WeakMethod(self.finish)   # model.settle(): the deferred apply, if any
        model._tgnx_invalidate = weakref.WeakMethod(self.invalidate_prefetch)
        model._tgnx_grow = weakref.WeakMethod(self.grow_nodes)   # model.grow_nodes(): the ring and bindings follow
        cfg = model.cfg
        if cfg.ring != loader.size:
            cfg.ring = loader.size
        self.cfg = cfg
        ev = {k: torch.as_tensor(v) for k, v in events.items()}
        model.ensure_events(int(ev["src"].numel()))
        self.src = ev["src"].to(self.dev, torch.long).contiguous()
        self.dst = ev["dst"].to(self.dev, torch.long).contiguous()
        self.t = ev["t"].to(self.dev, torch.float32).contiguous()
        self.msg = ev["msg"].to(self.dev, torch.float32).contiguous()
        if self.src.numel() > cfg.num_events:
            raise ValueError("event table larger than cfg.num_events")
        # the table's allocations (capacity rows; append_events grows them): src / dst / t / msg above are their first
        # num_events rows
        self._tab = (self.src, self.dst, self.t, self.msg)
        nb = _lib.lib().tgnx_tgn_ws_bytes(ctypes.byref(cfg))
        if nb == 0:
            raise RuntimeError(f"tgnx_tgn_ws_bytes: {_lib.lib().tgnx_last_error().decode()}")
        self.ws = torch.zeros(nb, dtype=torch.uint8, device=self.dev)
        self.ctl = torch.zeros(24, dtype=torch.int64, device=self.dev)   # TGNX_CTL_WORDS
        self.neg_train = torch.zeros(cfg.num_events, dtype=torch.long, device=self.dev)
        self.out_pos = torch.zeros(cfg.max_batch, dtype=torch.float32, device=self.dev)
        self.out_neg = torch.zeros(cfg.max_batch * max(cfg.max_neg, 1), dtype=torch.float32, device=self.dev)
        self.mrr = torch.zeros(cfg.max_batch, dtype=torch.float64, device=self.dev)
        self.out_ev = None    # optional per-event train-output log (tgnx_tgn_buffers.out_ev)
        # the bound split's plan table (tgnx_tgn_plan_table; resident parity-set steps read it), TGNX_PLAN_TABLE=0: off
        self.plan_table = None
        self.use_plan_table = os.environ.get("TGNX_PLAN_TABLE", "1") != "0"
        self.dst_nodes = None if dst_nodes is None else torch.as_tensor(dst_nodes).to(self.dev, torch.long).contiguous()
        self.seed, self.dp_rank, self.world = int(seed), int(rank), int(world)
        # the data-parallel step forms (exchange collective, then the apply + Adam launch): world > 1, or forced at
        # world 1 (data_parallel=True), where the exchange over a 1-rank group is an identity and the step must
        # equal the world-1 one (tests/test_gpu_tgn_rccl.py runs it through RCCL)
        self.dp = self.world > 1 if data_parallel is None else bool(data_parallel)
        if self.world > 1 and not self.dp:
            raise ValueError("TgnEngine: world > 1 needs the data-parallel step forms")
        self.fuse_adam = True
        # fused-Adam steps also store the gradient in model.grad_flat (grads_by_name); loops that never read it
        # (bench.py, the drop-in train()) set False before bind_resident: TGNX_TGN_NO_GRAD_STORE, 1.1 MB of
        # stores less per wiki-shaped step.  Data-parallel steps always write it (it is the exchange).
        self.keep_grads = True
        # parity-set steps gather the next batch's parameter-free message rows inside their fixup launch and start
        # with tgn_enc_fill instead of tgn_agg_emit (include/tgnx.h TGNX_TGN_NO_GATHER_AHEAD; the class docstring has
        # the rule for raw writes to memory between steps).  Set before bind_resident; False keeps tgn_agg_emit.
        self.gather_ahead = True
        # resident steps fold the batch cursor into the step's first launch: tgnx_tgn_train_step_resident
        # (world 1, Adam fused) or tgnx_tgn_train_fwd_bwd_resident (world > 1; exchange + update follow).
        # Both forms are tested against advance + step per rank (test_gpu_tgn.py, test_gpu_tgn_dp.py).
        self.fold_cursor = True
        # resident steps pipeline across steps (world 1: tgnx_tgn_train_step_pipelined; world > 1:
        # tgnx_tgn_train_fwd_bwd_pipelined, then the exchange and tgnx_tgn_apply_rows_update): each step marks
        # and scans the next batch, so the next step starts at the message aggregation.  `_prefetched` says
        # whether the last call on these buffers was such a step (any other call clears it).
        self.pipeline = True
        # world > 1 pipelined steps leave the next batch's scan out of fwd_bwd and run it while the exchange
        # is in flight (tgnx_tgn_train_fwd_bwd_split + tgnx_tgn_scan_next)
        self.split_scan = True
        # world-1 1-hop pipelined steps alternate two parities of the scan's per-batch outputs
        # (tgnx_tgn_train_step_pp): the next batch is scanned into the other set mid-step instead of in the
        # step's last launch; `_parity` = the set the next step reads (two captured graphs)
        self.parity_sets = os.environ.get("TGNX_PP", "1") != "0"   # (TGNX_PP=0: same-box A/B against the fold)
        self._parity = 0
        self._prefetched = False
        self._prefetch_version = None
        # data-parallel parity-set steps (tgnx_tgn_train_fwd_bwd_pp): the exchanged rows + Adam of step k run at
        # the head of step k + 1's graph; `_apply_pending` = the last step's exchange is not applied yet
        # (finish() applies it eagerly: before reading memory / parameters / the loss, and before any other call)
        self._apply_pending = False
        # the resident eval pass (bind_eval_resident): (split_lo, split_hi, batch, Kn), and its captured graphs
        # (single step, group size, group), held apart from the train graphs
        self._ev = None
        self._ev_graphs = None
        # the embedding table (enable_embedding_table; off by default): [node_capacity, D] current embeddings, the
        # stale planes T / D1 / D2 (tgnx_embtab.hip), `_emb_all` = every row is stale (set by every call that moves
        # state the host does not see batch by batch), and the (parameter, loader) versions the table was made at
        self._emb_tab = None
        self._emb_all = True
        self._emb_ver = None
        # the live pair history (enable_pair_history; off by default): a tgnx.pairset.PairSet that observe / eval
        # batches record into with one more launch
        self._pairs = None
        if optimizer is None:
            self.adam_m, self.adam_v = torch.zeros_like(model.flat), torch.zeros_like(model.flat)
        else:
            self.adam_m, self.adam_v = optimizer.exp_avg, optimizer.exp_avg_sq
        # data parallel: each rank's GRU-updated memory rows [node | last_update | memory]
        # travel with the gradients in ONE all-reduce over RCCL: the exchange buffer is [gradients |
        # world x xcap rows]; a rank writes only its own row slot (exact small-integer floats, the
        # other slots zero), so the sum of the row part is the all-gather.  tgnx_tgn_apply_rows writes
        # them into memory / last_update on every rank and zeroes the slots for the next step.
        self.xrows = self.xgather = self.comm = None
        # the exchange collective: torch.distributed.all_reduce over the default group, unless a callable
        # (comm, async_op) -> work | None is set here (tools/dp_compute.py: a stand-in without a collective)
        self.exchange = None
        # fused: one all-reduce of [gradients | row slots]; split: gradient all-reduce + row all-gather
        # (exchange_collectives; TGNX_EXCHANGE, for the first 8-GPU A/B of the two)
        self.exchange_mode = os.environ.get("TGNX_EXCHANGE", "fused")
        if self.exchange_mode not in EXCHANGE_MODES:
            raise ValueError(f"TGNX_EXCHANGE must be one of {EXCHANGE_MODES}, got {self.exchange_mode!r}")
        if self.dp:
            self.xcap = min(cfg.num_nodes, 2 * (-(-cfg.max_batch // self.world)))
            rw = cfg.mem_dim + 4
            G = model.grad_flat.numel()
            self.comm = torch.zeros(G + self.world * self.xcap * rw, dtype=torch.float32, device=self.dev)
            self.comm[:G].copy_(model.grad_flat)
            model.grad_flat = self.comm[:G]          # the kernels' gradient buffer heads the exchange buffer
            self.xgather = self.comm[G:].view(self.world * self.xcap, rw)
            self.xrows = self.xgather[self.dp_rank * self.xcap:(self.dp_rank + 1) * self.xcap]

    def ensure_neg(self, kn: int) -> None:
        """Grow the workspace for eval batches with kn negatives per event (TGB: ~999 on tgbl-wiki)."""
        if kn <= self.cfg.max_neg:
            return
        torch.cuda.synchronize(self.dev)
        self.cfg.max_neg = int(kn)
        nb = _lib.lib().tgnx_tgn_ws_bytes(ctypes.byref(self.cfg))
        if nb == 0:
            raise RuntimeError(f"tgnx_tgn_ws_bytes: {_lib.lib().tgnx_last_error().decode()}")
        self.ws = torch.zeros(nb, dtype=torch.uint8, device=self.dev)   # scratch only: zero = initial state
        self.out_neg = torch.zeros(self.cfg.max_batch * kn, dtype=torch.float32, device=self.dev)
        self._prefetched = False
        if hasattr(self, "_res_buf"):
            self._res_buf = self._buffers(_p(self.neg_train))
            self._buf_ref = ctypes.byref(self._res_buf)
        self._graphs = None                                   # captured pointers are stale
        self._rebind_eval()

    def _buffers(self, neg_ptr: int) -> TgnBuffers:
        m, ld = self.model, self.loader
        b = TgnBuffers()
        b.ev_src, b.ev_dst, b.ev_t, b.ev_msg = _p(self.src), _p(self.dst), _p(self.t), _p(self.msg)
        b.neg = neg_ptr
        b.dst_nodes = _p(self.dst_nodes)
        b.n_dst = 0 if self.dst_nodes is None else self.dst_nodes.numel()
        b.nbr, b.eid, b.rt, b.assoc = _p(ld.neighbors), _p(ld.e_id), _p(ld.t), _p(ld._assoc)
        b.memory, b.last_update = _p(m.memory.memory), _p(m.memory.last_update)
        b.store, b.node_gen = _p(m.store), _p(m.node_gen)
        b.params, b.grads, b.adam_m, b.adam_v = _p(m.flat), _p(m.grad_flat), _p(self.adam_m), _p(self.adam_v)
        b.ctl, b.out_pos, b.out_neg, b.mrr, b.ws = _p(self.ctl), _p(self.out_pos), _p(self.out_neg), _p(self.mrr), _p(self.ws)
        b.xrows, b.xcap = _p(self.xrows), (0 if self.xrows is None else self.xcap)
        b.out_ev = _p(self.out_ev)
        b.plan_table = _p(self.plan_table)
        b.flags = (0 if self.keep_grads else 1) | (0 if self.gather_ahead else 2)   # TGNX_TGN_NO_GRAD_STORE, _NO_GATHER_AHEAD
        # steps on these buffers leave grad_flat stale (fused Adam without the store; data-parallel steps always
        # write it: it heads the exchange buffer)
        m._grads_stale = not self.keep_grads and not self.dp
        return b

    def _stream(self):
        return _lib.stream(self.dev)

    def invalidate_prefetch(self):
        """The next resident step marks, scans and gathers its batch itself (model.invalidate_prefetch)."""
        self._prefetched = False

    def _settle(self):
        """Every call that reads or rewrites the state runs this first: a deferred data-parallel apply lands now, and
        the next train step prepares its batch itself."""
        self.finish()
        self._prefetched = False

    def advance(self, batch_start: int, B: int, train: bool):
        self._settle()
        _lib.call("tgnx_tgnn_advance", _p(self.ctl), 0, batch_start, B, batch_start, 0, 0, 1, self.dp_rank, self.world,
                  self.seed, 1 if train else 0, self._stream())

    # ------------------------------------------------------------------ state
    def reset_state(self):
        """memory_module.reset_state + neighbor_loader.reset_state (pyg_epoch_utils.py:15-16)."""
        self._settle()
        self._emb_all = True
        b = self._buffers(0)
        _lib.call("tgnx_tgn_reset_state", ctypes.byref(self.cfg), ctypes.byref(b), self._stream())
        self.loader.reset_state()
        if self._pairs is not None:       # (the stream starts over: its rows will be observed again)
            self._pairs.clear()

    def flush(self):
        """TGNMemory.train(False) (memory_module.py:209-215)."""
        self._settle()
        self._emb_all = True
        b = self._buffers(0)
        nb = int(_lib.lib().tgnx_tgn_flush_scratch_bytes(ctypes.byref(self.cfg)))
        # graphs beyond one workspace chunk: a snapshot of memory / last_update.  It is allocated on, and
        # the flush runs on, the current stream, so the caching allocator reuses the block only for work
        # queued after the flush: it may go out of scope when this call returns
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.dev) if nb else None
        _lib.call("tgnx_tgn_flush", ctypes.byref(self.cfg), ctypes.byref(b), _p(scratch), nb, self._stream())

    # ------------------------------------------------------------------ steps
    def train_batch(self, start: int, B: int, neg=None, dropout: bool = True, update: bool = True):
        """One TGN train batch over events [start, start + B).  neg: LongTensor[B] to inject, or None to
        draw on the device.  Returns (sigmoid(pos), sigmoid(neg)) views."""
        if neg is not None:
            self.neg_train[start:start + B].copy_(torch.as_tensor(neg).to(self.dev, torch.long))
        self.advance(start, B, True)
        self._emb_all = True
        b = self._buffers(_p(self.neg_train))
        fused = update and self._fused()
        _lib.call("tgnx_tgn_train_step" if fused else "tgnx_tgn_train_fwd_bwd", ctypes.byref(self.cfg), ctypes.byref(b),
                  0 if neg is not None else 1, 1 if dropout else 0, self._stream())
        self._pending = b
        if update and not fused:
            self.apply_update()
        return self.out_pos[:B], self.out_neg[:B]

    def _fused(self) -> bool:
        """Adam folded into the step's gradient writers (tgnx_tgn_train_step): world 1 only, since data
        parallel steps all-reduce the gradients before the update."""
        return self.fuse_adam and not self.dp

    def apply_update(self, allreduce: bool = True):
        self._emb_all = True
        if allreduce and self.dp:
            self._exchange()
        if self.dp:   # the exchanged rows and Adam in one launch
            _lib.call("tgnx_tgn_apply_rows_update", ctypes.byref(self.cfg), ctypes.byref(self._pending),
                      _p(self.xgather), self.xgather.shape[0], self._stream())
        else:
            _lib.call("tgnx_tgn_train_update", ctypes.byref(self.cfg), ctypes.byref(self._pending), self._stream())

    def _exchange(self):
        """The step's one collective: gradient sum and the touched memory rows of every rank (an
        all-gather carried by the same all-reduce, see __init__)."""
        if self.exchange is not None:
            self.exchange(self.comm, False)
            return
        exchange_collectives(self.comm, self.model.grad_flat.numel(), self.dp_rank, self.world, self.exchange_mode)

    def _apply_rows(self, b):
        _lib.call("tgnx_tgn_apply_rows", ctypes.byref(self.cfg), ctypes.byref(b), _p(self.xgather),
                  self.xgather.shape[0], self._stream())

    def eval_batch(self, start: int, B: int, negs):
        """TGB-style eval batch: negs LongTensor[B, Kn].  Returns (pos [B], neg [B, Kn], rr [B])."""
        negs = torch.as_tensor(negs).to(self.dev, torch.long).contiguous()
        Kn = negs.shape[1]
        self.ensure_neg(Kn)
        self.advance(start, B, False)
        # the kernels index neg[(start + i) * Kn + c]: shift the base pointer by start rows
        b = self._buffers(negs.data_ptr() - start * Kn * 8)
        _lib.call("tgnx_tgn_eval_step", ctypes.byref(self.cfg), ctypes.byref(b), Kn, self._stream())
        self._emb_touch(start, B)
        self._pairs_touch(start, B)
        self._keep = negs
        return self.out_pos[:B], self.out_neg[:B * Kn].view(B, Kn), self.mrr[:B]

    # ------------------------------------------------------------------ score-free ingestion
    @property
    def num_events(self) -> int:
        """Valid rows of the event table (cfg.num_events is its capacity, which sizes the store arena)."""
        return int(self.src.numel())

    @property
    def event_capacity(self) -> int:
        return int(self._tab[0].numel())

    def _set_rows(self, n: int):
        self.src, self.dst, self.t, self.msg = (x[:n] for x in self._tab)

    def reserve_events(self, n: int) -> None:
        """Capacity for at least n event rows, ahead of time (append_events grows it geometrically otherwise).  On
        growth the four table tensors are reallocated and copied, the model's store arena grows with them
        (TGNModel.ensure_events keeps the stored words), neg_train and the output log are resized, cfg.num_events
        follows the capacity, and everything that captured a pointer is dropped as ensure_neg drops it: the resident
        binding is made again (its plan table rebuilt), the captured train and eval graphs are gone (capture again)."""
        n = int(n)
        old = self._tab
        if n <= old[0].numel():
            return
        self.finish()
        torch.cuda.synchronize(self.dev)
        rows = self.num_events
        new = tuple(torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.dev) for x in old)
        for a, b in zip(new, old):
            a[:rows].copy_(b[:rows])
        self._tab = new
        self._set_rows(rows)
        self.model.ensure_events(n)
        cap = int(self.cfg.num_events)
        for name in ("neg_train", "out_ev"):
            x = getattr(self, name)
            if x is not None and x.shape[0] < cap:
                y = torch.zeros((cap,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.dev)
                y[:x.shape[0]].copy_(x)
                setattr(self, name, y)
        self._prefetched = False
        self._graphs = None                                   # captured pointers are stale
        self._group = None
        if hasattr(self, "_res_buf"):
            self.bind_resident(*self._res, dropout=bool(self._res_drop))   # (drops and rebuilds the plan table)
        else:
            self._rebind_eval()

    # ------------------------------------------------------------------ a node space that grows
    @property
    def node_capacity(self) -> int:
        """Rows allocated under every [N, .] tensor (>= cfg.num_nodes, the logical node count; capacity rows are
        reset rows no call reads: never candidates, never counted, not in stream_state())."""
        return min(self.model.node_capacity, self.loader.node_capacity)

    @torch.no_grad()
    def _grow(self, n: int, cap: int) -> int:
        """The node space at max(n, N) nodes over allocations of at least `cap` rows (grow_nodes / reserve_nodes)."""
        m, ld, cfg = self.model, self.loader, self.cfg
        N, have = int(cfg.num_nodes), self.node_capacity
        n = max(int(n), N)
        cap = max(int(cap), n, have)
        if n == N and cap == have:
            return N
        if ld.num_nodes != N:
            raise ValueError(f"grow_nodes: the loader holds {ld.num_nodes} nodes, the model {N}")
        nb = 0
        if cap < MAX_NODES:
            probe = TgnConfig.from_buffer_copy(cfg)
            probe.num_nodes = n
            nb = int(_lib.lib().tgnx_tgn_ws_bytes(ctypes.byref(probe)))
        if nb == 0:
            raise ValueError(f"grow_nodes: {n} nodes (capacity {cap}) are beyond what the node id type and "
                             "tgnx_tgn_ws_bytes accept")
        self._settle()
        torch.cuda.synchronize(self.dev)
        old = dict(nbr=ld.neighbors, eid=ld.e_id, rt=ld.t, assoc=ld._assoc, memory=m.memory.memory,
                   last_update=m.memory.last_update, node_gen=m.node_gen, store=m.store)
        rows = cap > have
        new = grow_node_tensors(self.dev, N, n, cap, cfg.ring, cfg.mem_dim, cfg.num_events, old, rows=rows)
        # (a store run outside the arena has raised by now, with nothing swapped)
        if rows:
            ring, node = tuple(new[k] for k in ("nbr", "eid", "rt", "assoc")), \
                tuple(new[k] for k in ("memory", "last_update", "node_gen"))
        else:
            ring, node = ld._alloc, m._node_alloc
        lv = getattr(ld, "version", None)
        ld._install(*ring, n)
        m._install_nodes(*node, new.get("store", m.store), n)
        self._emb_moved(N, lv)
        if n > N:   # the workspace's layout follows num_nodes: a fresh one (scratch only: zero = initial state)
            self.ws = torch.zeros(nb, dtype=torch.uint8, device=self.dev)
        self._prefetched = False
        self._graphs = None                                   # captured pointers (and the captured N) are stale
        self._group = None
        for a in ("_pending", "_keep"):
            self.__dict__.pop(a, None)
        if hasattr(self, "_res_buf"):
            self.bind_resident(*self._res, dropout=bool(self._res_drop))   # (drops and rebuilds the plan table)
        else:
            self._release_plan_table()
            self._rebind_eval()
        return n

    def reserve_nodes(self, cap: int) -> None:
        """Row capacity for at least cap nodes ahead of time (append_events(grow=True) grows it geometrically
        otherwise): the [N, .] tensors move into allocations of cap rows, cfg.num_nodes stays.  Pointers change, so
        graphs and bindings are treated as grow_nodes treats them."""
        check_grow_args(self.cfg.num_nodes, cap, self.world, self.dp)
        self._grow(self.cfg.num_nodes, cap)

    def grow_nodes(self, n: int) -> int:
        """Extend the node space to n nodes in place; returns cfg.num_nodes afterwards (n <= N: a no-op returning N).
        The result is bit for bit the state of an engine built at n nodes and fed the same calls: rows [0, N) of
        memory, last_update, node_gen, the ring (neighbors, e_id, t, _assoc), the store's node table and every arena
        entry are unchanged; rows [N, n) are what reset_state leaves on a fresh engine (memory 0, last_update 0,
        node_gen 0, neighbors -1, e_id -1, t -1.0, empty store runs); no parameter, Adam moment, ctl word (GEN and
        ERR included) or event row changes.  The tensors move into allocations of node_capacity >= n rows when the
        capacity is exceeded (tgnx_tgn_grow_nodes), the store is re-laid for every growth (its arena sits 4 * N
        words in), and the workspace is a fresh zero one.  Everything that captured a pointer is dropped as
        reserve_events / ensure_neg drop it: the captured train and eval graphs, the plan table, the prefetched
        batch; the resident train and eval bindings are made again (their rows still exist; the eval cursor and its
        reciprocal ranks are kept), so capture again and go on.  loader.version is bumped.
        Every default that means "all nodes" (recommend / rank candidates, embed's id check, the train negatives'
        range without dst_nodes) follows cfg.num_nodes.  A dst_nodes the caller passed is NOT extended: the train
        negative pool and the default candidates are the caller's statement.
        n beyond what the id type and tgnx_tgn_ws_bytes accept: ValueError before anything is touched; a store run
        outside the arena: RuntimeError, the engine untouched.  One device only (ValueError at world > 1 / dp).
        One host read."""
        if not check_grow_args(self.cfg.num_nodes, n, self.world, self.dp):
            return int(self.cfg.num_nodes)
        return self._grow(n, n)

    @torch.no_grad()
    def append_events(self, src, dst, t, msg, validate: bool = True):
        """Append rows to the device event table; returns (start, n): they are rows [start, start + n).  dtypes are
        converted as the constructor converts them; msg must be [n, msg_dim].  validate: one host read checks the
        node ids against [0, N) and raises ValueError before anything is written; without it (no host read) ids are
        clamped into [0, N), so an id out of range never reaches a kernel as an index.  Appending alone moves no
        stream state: observe() / observe_range() / eval and train batches over the new rows do.  Ids of nodes that
        do not exist yet: append_events_grow()."""
        return self._append(src, dst, t, msg, validate, False)

    @torch.no_grad()
    def append_events_grow(self, src, dst, t, msg):
        """append_events for rows that may name new nodes: an id >= N is not an error — the host read that validation
        makes takes the largest id instead (one device min / max over src and dst) and the node space grows to it + 1
        first (grow_nodes semantics, capacity by grown_node_capacity).  Negative ids are still a ValueError."""
        return self._append(src, dst, t, msg, True, True)

    def _append(self, src, dst, t, msg, validate: bool, grow: bool):
        check_append_args(validate, grow)
        src = torch.as_tensor(src).to(self.dev, torch.long).contiguous().view(-1)
        dst = torch.as_tensor(dst).to(self.dev, torch.long).contiguous().view(-1)
        t = torch.as_tensor(t).to(self.dev, torch.float32).contiguous().view(-1)
        msg = torch.as_tensor(msg).to(self.dev, torch.float32).contiguous()
        n = check_event_rows(src.numel(), dst.numel(), t.numel(), tuple(msg.shape), self.cfg.msg_dim)
        N = self.cfg.num_nodes
        if grow:
            check_grow_args(N, N, self.world, self.dp)
            if n:
                lo, hi = torch.stack([torch.minimum(src.min(), dst.min()), torch.maximum(src.max(), dst.max())]).tolist()
                if lo < 0:
                    raise ValueError("append_events: node ids must not be negative")
                if hi >= N:
                    self._grow(hi + 1, grown_node_capacity(self.node_capacity, hi + 1))
        elif validate:
            if n and bool(((src < 0) | (src >= N) | (dst < 0) | (dst >= N)).any()):
                raise ValueError(f"append_events: node ids must be in [0, {N})")
        else:
            src, dst = src.clamp(0, N - 1), dst.clamp(0, N - 1)
        start = self.num_events
        if n == 0:
            return start, 0
        self._settle()
        self.reserve_events(grown_capacity(self.event_capacity, start + n))
        for buf, rows in zip(self._tab, (src, dst, t, msg)):
            buf[start:start + n].copy_(rows)
        self._set_rows(start + n)
        return start, n

    def observe(self, start: int, B: int):
        """Advance memory, last_update, the message stores and the ring over resident rows [start, start + B) without
        scoring anything (tgnx_tgn_observe_step): the state afterwards is what eval_batch(start, B, negs) leaves for
        any negatives.  No negatives, no outputs.  Asynchronous like every step: check() reads the error flags."""
        start, B = int(start), int(B)
        check_observe_args(start, B, self.cfg.max_batch, self.num_events, self.world)
        self.advance(start, B, False)
        b = self._buffers(0)
        b.xrows, b.xcap = 0, 0
        _lib.call("tgnx_tgn_observe_step", ctypes.byref(self.cfg), ctypes.byref(b), self._stream())
        self._emb_touch(start, B)
        self._pairs_touch(start, B)

    def observe_range(self, lo: int, hi: int, batch=None):
        """observe() over resident rows [lo, hi) in batches of `batch` (default cfg.max_batch), the last one partial:
        the replay that rebuilds memory, stores and ring from history — after loading a checkpoint, say — without
        scoring negatives.  Batching is semantic in TGN (the messages of one batch do not see each other): the result
        is that of an eval pass over the same rows with the same batching."""
        lo, hi = int(lo), int(hi)
        batch = int(self.cfg.max_batch if batch is None else batch)
        if not (0 <= lo <= hi <= self.num_events) or not (0 < batch <= self.cfg.max_batch):
            raise ValueError(f"observe_range: rows [{lo}, {hi}) batch {batch} outside the event table "
                             f"({self.num_events} events) / max_batch ({self.cfg.max_batch})")
        for a in range(lo, hi, batch):
            self.observe(a, min(batch, hi - a))

    def observe_events(self, src, dst, t, msg, batch=None, validate: bool = True, grow: bool = False):
        """append_events, then observe the new rows in batches of `batch` (default cfg.max_batch) — batched per call:
        two calls of 30 events at batch 50 are two batches of 30.  grow: nodes that first appear in these rows are
        admitted (append_events_grow; grow without validate is a ValueError: growing needs validation's host read).
        Returns (start, n)."""
        if self.world > 1:
            raise ValueError("observe_events: one device only (world > 1 is not built)")
        start, n = self._append(src, dst, t, msg, validate, grow)
        self.observe_range(start, start + n, batch)
        return start, n

    # ------------------------------------------------------------------ compaction and stream-state checkpoints
    def _drop_bindings(self):
        """Forget everything that captured a pointer or names a row range: the captured train and eval graphs, the
        plan table, the resident train and eval bindings (not made again: the caller binds again) and the drop-in
        loops' record of what they bound."""
        self._prefetched = False
        self._graphs = None
        self._group = None
        self._release_plan_table()
        for a in ("_res_buf", "_buf_ref", "_res", "_res_drop", "_res_fused", "_f", "_cfg_ref", "_ctl_p", "_pending",
                  "_ev_buf", "_ev_buf_ref", "_ev_negs", "_ev_rr", "_keep", "_pair_hist"):
            self.__dict__.pop(a, None)
        self._ev = None
        self._ev_graphs = None
        for a in ("_bound", "_eval_bound"):          # (tgn_epoch.train / test: bind again on their next call)
            if a in self.__dict__:
                setattr(self, a, None)

    def _install_table(self, tab, rows: int, store: torch.Tensor):
        """Fresh table allocations of capacity tab[0].shape[0] with `rows` valid rows, and a fresh store sized for it:
        cfg.num_events, neg_train and out_ev follow the capacity (re-zeroed: their rows belong to the old numbering)."""
        cap = int(tab[0].shape[0])
        m = self.model
        self._tab = tuple(tab)
        self._set_rows(rows)
        m.store = store
        m.cfg.num_events = m.num_events = cap
        self.neg_train = torch.zeros(cap, dtype=torch.long, device=self.dev)
        if self.out_ev is not None:
            self.out_ev = torch.zeros((cap,) + tuple(self.out_ev.shape[1:]), dtype=self.out_ev.dtype, device=self.dev)
        self.loader.cur_e_id = rows
        self.loader.version = getattr(self.loader, "version", 0) + 1

    def _compact_plan(self, upto: int):
        """tgnx_tgn_compact_plan over the current table; returns (workspace, n_live, live arena entries, bad ids)
        after one host read.  Writes only the workspace."""
        nev = self.num_events
        nb = int(_lib.lib().tgnx_tgn_compact_ws_bytes(ctypes.byref(self.cfg), nev))
        if nb == 0:
            raise RuntimeError(f"tgnx_tgn_compact_ws_bytes: {_lib.lib().tgnx_last_error().decode()}")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)
        _lib.call("tgnx_tgn_compact_plan", ctypes.byref(self.cfg), ctypes.byref(self._buffers(0)), nev, int(upto), _p(ws),
                  nb, self._stream())
        rec = ws[:64].view(torch.int64).tolist()
        return ws, int(rec[0]), int(rec[1]), int(rec[2])

    def _compact_apply(self, ws: torch.Tensor, n_live: int, cap: int) -> torch.Tensor:
        """tgnx_tgn_compact_apply into fresh allocations of `cap` rows, then the engine's tensors are swapped."""
        old, N = self._tab, self.cfg.num_nodes
        new = tuple(torch.zeros((cap,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.dev) for x in old)
        store = torch.zeros(4 * N + 2 * cap, dtype=torch.long, device=self.dev)
        kept = torch.empty(n_live, dtype=torch.long, device=self.dev)
        keep = torch.empty(1, dtype=torch.long, device=self.dev) if n_live == 0 else kept   # (a non-null pointer)
        _lib.call("tgnx_tgn_compact_apply", ctypes.byref(self.cfg), ctypes.byref(self._buffers(0)), self.num_events, cap,
                  _p(new[0]), _p(new[1]), _p(new[2]), _p(new[3]), _p(store), _p(keep), n_live, _p(ws), ws.numel(),
                  self._stream())
        self._install_table(new, n_live, store)
        return kept

    @torch.no_grad()
    def compact_events(self, upto=None, capacity=None) -> torch.Tensor:
        """Retire every row of the device event table that nothing references and renumber the survivors in order
        (new id = rank among the live rows).  Returns kept, a LongTensor [n_live] of the surviving rows' old ids
        (kept[new] = old), with which a caller translates its own records.

        A row is kept if a ring slot with neighbors != -1 holds its id, if a node's s- or d-store run holds it, or if
        its id is >= upto (default num_events).  Rows >= upto are kept verbatim whether referenced or not: that is how
        a caller protects rows it has appended but not observed yet — pass upto = the first unobserved row; without it
        such rows are retired like any other unreferenced row.

        Afterwards num_events == n_live; the four table tensors and model.store are fresh allocations of `capacity`
        rows (>= n_live, ValueError otherwise) or, by default, of grown_capacity's max(n_live + 1, 1.5 x n_live);
        cfg.num_events, neg_train and out_ev follow the capacity (re-zeroed); loader.cur_e_id = n_live and
        loader.version is bumped; ctl BATCH_START = CUR_EID = n_live, no other ctl word changes.  memory, last_update,
        node_gen and the parameters are untouched; what the ring and the stores name is unchanged.  Like
        reserve_events, everything that captured a pointer or names a row range is dropped — the captured train and
        eval graphs, the plan table, and the resident train and eval bindings, which are NOT made again (their rows no
        longer exist): bind again.  Train negatives drawn on the device after a compaction differ from an uncompacted
        engine's (their RNG offset is the batch's CUR_EID).  The old and new tables coexist until this returns.

        An event id outside [0, num_events) in the ring or a store is counted on the device, never dereferenced:
        RuntimeError, with the engine untouched.  One device only (ValueError at world > 1).  One host read.

        The embedding table (enable_embedding_table) stays current: ids are renumbered, but every ring slot and store
        entry names a row with the same t and msg values, and an embedding reads values, not ids: nothing goes stale."""
        upto = check_compact_args(self.num_events, upto, capacity, self.world)
        if self.dp:
            raise ValueError("compact_events: one device only (the data-parallel step forms are not built)")
        self._settle()
        ws, n_live, n_arena, n_bad = self._compact_plan(upto)
        if n_bad:
            raise RuntimeError(f"compact_events: {n_bad} event ids / store runs outside the table's {self.num_events} "
                               "rows in the ring or the message stores; nothing was changed")
        if n_arena > 2 * n_live:
            raise RuntimeError(f"compact_events: the stores hold {n_arena} entries for {n_live} live rows (an event "
                               "twice in one run); nothing was changed")
        cap = compact_capacity(n_live, capacity)
        self._drop_bindings()
        lv = getattr(self.loader, "version", None)
        kept = self._compact_apply(ws, n_live, cap)
        self._emb_moved(self.cfg.num_nodes, lv)
        return kept

    # ------------------------------------------------------------------ forgetting nodes
    def _forget_plan(self, ids: torch.Tensor):
        """tgnx_tgn_forget_plan for the id tensor; returns (workspace, record as a list of 8 ints) after one host
        read.  Writes only the workspace."""
        nb = int(_lib.lib().tgnx_tgn_forget_ws_bytes(ctypes.byref(self.cfg)))
        if nb == 0:
            raise RuntimeError(f"tgnx_tgn_forget_ws_bytes: {_lib.lib().tgnx_last_error().decode()}")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)
        _lib.call("tgnx_tgn_forget_plan", ctypes.byref(self.cfg), ctypes.byref(self._buffers(0)), self.num_events,
                  _p(ids), ids.numel(), _p(ws), nb, self._stream())
        return ws, ws[:64].view(torch.int64).tolist()

    def _forget_apply(self, ws: torch.Tensor) -> None:
        """Drop the bindings, bump loader.version and run tgnx_tgn_forget_apply on a clean plan's workspace."""
        self._drop_bindings()
        lv = getattr(self.loader, "version", 0)
        self.loader.version = lv + 1
        flags = self._emb_flags if self._emb_tab is not None else None
        _lib.call("tgnx_tgn_forget_apply", ctypes.byref(self.cfg), ctypes.byref(self._buffers(0)), self.num_events,
                  _p(ws), ws.numel(), _p(flags), self._stream())
        # (the table's record of the loader version follows: only the marked rows are stale)
        self._emb_moved(int(self.cfg.num_nodes), lv)

    @torch.no_grad()
    def forget_nodes(self, ids, *, compact: bool = False, drop_candidates: bool = False) -> dict:
        """Erase the nodes `ids` (any integer sequence / tensor; duplicates allowed) from the stream state in place.

        Own rows: memory, last_update and node_gen of a forgotten node become 0, its store runs empty and its ring row
        neighbors -1 / e_id -1 / t -1.0 — bit for bit the row grow_nodes gives a node that has never been seen.  Other
        nodes: every valid ring slot (e_id >= 0 and neighbors != -1) that names a forgotten node is removed, the row's
        surviving (e_id, neighbors) pairs keep their order at the front and the rest of the row becomes (-1, -1); its
        t column becomes ev_t[e_id] of the survivors ranked descending (ties by slot) with -1.0 behind them — on a
        time-ordered stream that is the old column without the removed slots, on a stream whose t is shuffled it
        repairs the column to the kept events' times.  Every store entry whose event has a forgotten node at the
        other end is dropped and the run packed in place (offset kept, count reduced; an emptied run becomes {0, 0}).
        A ring row or run that loses nothing is not written.  Nothing else moves: ctl, the batch cursor, parameters,
        Adam moments and the event table stay; the rows only the forgotten nodes kept alive are dead, and
        compact_events() (compact=True runs it straight away, with its default upto) retires every observed row with
        an endpoint in ids.  Rows appended but not observed yet are not examined: filter them before observing, and
        note that a default compaction retires them (compact_events: upto).

        What is NOT undone: a partner's memory vector has already folded the node's past messages in through the
        memory updater, and the parameters were trained on its events.  Nothing is retrained or recomputed.

        The node stays in the node space: ids are not renumbered and it may be observed again (an id reused).  It
        also stays a default candidate of recommend / rank and a train negative, scoring as a never-seen node does,
        unless drop_candidates=True removes ids from dst_nodes (None becomes every node but ids; one more host read
        for the mask select; ValueError, with nothing changed, if no candidate would be left).

        Returns {"nodes": distinct ids, "ring_slots": slots removed from other nodes' rows, "ring_rows": rows that
        lost one, "store_entries": entries dropped from other nodes' runs}, and "kept" (compact_events' result) with
        compact=True.  With the pair history enabled (enable_pair_history) every pair that names a forgotten node is
        erased as well and "pairs" counts them (three more host reads); the key is absent otherwise.  An empty id list
        is a no-op: zeros, nothing launched, compacted or dropped.

        Like compact_events, everything that captured a pointer or names a batch prepared from the old state is
        dropped — the captured train and eval graphs, the plan table, the resident train and eval bindings (not made
        again): bind again.  loader.version is bumped.  With the embedding table enabled, the forgotten nodes and the
        rewritten ring rows are marked stale; the next refresh re-embeds them and their ring dependents only.

        An id outside [0, N): ValueError.  A ring slot, store run or arena entry that names an event or node out of
        range is counted on the device, never dereferenced: RuntimeError.  Both with the engine untouched.  One
        device only (ValueError at world > 1 / the data-parallel forms).  One host read (two on the error path)."""
        ids = self._ids(ids)
        if not check_forget_args(self.cfg.num_nodes, ids.numel(), self.world, self.dp):
            return dict.fromkeys(FORGET_COUNTS + (("pairs",) if self._pairs is not None else ()), 0)
        self._settle()
        N = int(self.cfg.num_nodes)
        ws, rec = self._forget_plan(ids)
        if rec[4]:
            if bool(((ids < 0) | (ids >= N)).any()):
                raise ValueError(f"forget_nodes: node ids must be in [0, {N}); nothing was changed")
            raise RuntimeError(f"forget_nodes: {rec[4]} event ids / node ids / store runs out of range in the ring or "
                               "the message stores; nothing was changed")
        pool = None
        if drop_candidates:
            pool = torch.arange(N, device=self.dev) if self.dst_nodes is None else self.dst_nodes
            pool = pool[~torch.isin(pool, ids)].contiguous()
            if pool.numel() == 0:
                raise ValueError("forget_nodes: drop_candidates would leave no candidate; nothing was changed")
        self._forget_apply(ws)
        if pool is not None:
            self.dst_nodes = pool
        out = {k: int(rec[i]) for i, k in enumerate(FORGET_COUNTS)}
        if self._pairs is not None:       # every pair that names a forgotten node (tgnx_pairset_rehash with flags)
            out["pairs"] = self._pair_set("forget_nodes").erase_nodes(ids)
        if compact:
            out["kept"] = self.compact_events()
        return out

    @torch.no_grad()
    def stream_state(self) -> dict:
        """The whole stream state as a flat dict of cloned tensors and plain ints (STREAM_STATE_KEYS): format = 1, the
        fingerprint num_nodes / ring / mem_dim / msg_dim, num_events, the table rows [0, num_events), memory,
        last_update, node_gen, the stores' node table and arena entries [0, 2 * num_events), the ring and the ctl
        block.  No parameters: model.state_dict() has them.  Round-trips through torch.save / torch.load; small when
        taken after compact_events(), valid without one."""
        if self.world > 1:
            raise ValueError("stream_state: one device only (world > 1 is not built)")
        self.finish()
        m, ld, N, n = self.model, self.loader, self.cfg.num_nodes, self.num_events
        out = dict(format=STREAM_STATE_FORMAT, **stream_fingerprint(self.cfg), num_events=n)
        tensors = dict(src=self.src, dst=self.dst, t=self.t, msg=self.msg, memory=m.memory.memory,
                       last_update=m.memory.last_update, node_gen=m.node_gen, store_nodes=m.store[:4 * N].view(N, 4),
                       store_arena=m.store[4 * N:4 * N + 2 * n], neighbors=ld.neighbors, e_id=ld.e_id, ring_t=ld.t,
                       ctl=self.ctl)
        out.update({k: tensors[k].detach().clone() for k in STREAM_STATE_TENSORS})
        return out

    @torch.no_grad()
    def load_stream_state(self, state: dict) -> None:
        """Make a stream_state() dict this engine's stream state, whatever table the engine was built over (one row
        is enough).  format, the fingerprint, the shapes and ERR == 0 in the saved ctl are checked first: ValueError
        before anything is written.  Table and store are sized by reserve_events, everything is copied in,
        loader.cur_e_id = num_events, and bindings and graphs are dropped as compact_events drops them.  Keys beyond
        STREAM_STATE_KEYS (a save_stream file's "pair_history") are ignored.  A state of another node count:
        load_stream_state_grow()."""
        self._load_stream_state(state, False)

    @torch.no_grad()
    def load_stream_state_grow(self, state: dict) -> None:
        """load_stream_state for a state whose num_nodes may differ from the engine's (check_stream_state_grow: nothing
        else is relaxed).  A state of more nodes grows the engine first (grow_nodes); a state of fewer nodes is loaded
        into the first rows and the engine's other rows become reset rows (as grow_nodes would have left them)."""
        self._load_stream_state(state, True)

    def _load_stream_state(self, state: dict, grow: bool) -> None:
        if self.world > 1:
            raise ValueError("load_stream_state: one device only (world > 1 is not built)")
        if grow:
            n, ns = check_stream_state_grow(state, stream_fingerprint(self.cfg))
        else:
            n, ns = check_stream_state(state, stream_fingerprint(self.cfg)), int(self.cfg.num_nodes)
        err = int(state["ctl"][11])
        if err:
            raise ValueError(f"load_stream_state: the saved ctl block carries step error flags {err:#x}")
        if ns > self.cfg.num_nodes:
            self.grow_nodes(ns)
        self.finish()
        self._drop_bindings()
        self.reserve_events(max(n, 1))
        torch.cuda.synchronize(self.dev)
        for buf, k in zip(self._tab, ("src", "dst", "t", "msg")):
            buf[:n].copy_(state[k].to(self.dev, buf.dtype))
        self._set_rows(n)
        m, ld, N = self.model, self.loader, self.cfg.num_nodes
        m.store[:4 * ns].copy_(state["store_nodes"].to(self.dev, torch.long).reshape(-1))
        m.store[4 * ns:4 * N].zero_()                       # (ns < N: empty runs for the nodes the state lacks)
        m.store[4 * N:4 * N + 2 * n].copy_(state["store_arena"].to(self.dev, torch.long))
        for dst, k, reset in ((m.memory.memory, "memory", 0), (m.memory.last_update, "last_update", 0),
                              (m.node_gen, "node_gen", 0), (ld.neighbors, "neighbors", -1), (ld.e_id, "e_id", -1),
                              (ld.t, "ring_t", -1.0)):
            dst[:ns].copy_(state[k].to(self.dev, dst.dtype))
            dst[ns:].fill_(reset)
        self.ctl.copy_(state["ctl"].to(self.dev, self.ctl.dtype))
        ld.cur_e_id = n
        ld.version = getattr(ld, "version", 0) + 1
        self._emb_all = True

    # ------------------------------------------------------------------ read-only inference
    def embed_capacity(self) -> int:
        """Nodes per tgnx_tgn_embed call: the eval root capacity min(N, max_batch * (2 + max_neg))."""
        return int(_lib.lib().tgnx_tgn_embed_max_nodes(ctypes.byref(self.cfg)))

    # ------------------------------------------------------------------ the embedding table
    def enable_embedding_table(self) -> None:
        """Keep a materialised [node_capacity, D] table of current eval-mode embeddings (off by default): queries with
        cached=True read it instead of embedding their nodes again, and refresh_embeddings() recomputes only the rows
        the batches since the last refresh made stale — their endpoints T and the nodes with a node of T in a valid
        ring slot (two hops of that at layers = 2; include/tgnx.h has the rule).  Allocates the table and the stale
        planes with every row stale.  While enabled, observe / eval batches pay one more launch (tgnx_embtab_touch).
        One device only (ValueError at world > 1 / dp)."""
        if self.world > 1 or self.dp:
            raise ValueError("enable_embedding_table: one device only (world > 1 is not built)")
        if self._emb_tab is None:
            self._emb_alloc(max(self.node_capacity, int(self.cfg.num_nodes)))
            self._emb_all = True

    def disable_embedding_table(self) -> None:
        """Free the table and the planes; every call issues exactly the launches it issues without the feature."""
        self._emb_tab = self._emb_flags = self._emb_ids = self._emb_cnt = self._emb_ws = None

    def _emb_alloc(self, cap: int) -> None:
        nb = int(_lib.lib().tgnx_embtab_list_ws_bytes(cap))
        if nb == 0:
            raise RuntimeError(f"tgnx_embtab_list_ws_bytes: {cap} nodes are beyond the node id type")
        self._emb_tab = torch.zeros(cap, self.cfg.mem_dim, dtype=torch.float32, device=self.dev)
        self._emb_flags = torch.zeros(3 * cap, dtype=torch.uint8, device=self.dev)   # planes [3][N], N = cfg.num_nodes
        self._emb_ids = torch.empty(cap, dtype=torch.long, device=self.dev)
        self._emb_cnt = torch.zeros(1, dtype=torch.long, device=self.dev)
        self._emb_ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)

    def _emb_touch(self, start: int, B: int) -> None:
        """Mark the endpoints of event rows [start, start + B) stale (nothing to do while every row is)."""
        if self._emb_tab is None or self._emb_all or B <= 0:
            return
        _lib.call("tgnx_embtab_touch", self._tab[0].data_ptr() + start * 8, self._tab[1].data_ptr() + start * 8, B,
                  int(self.cfg.num_nodes), _p(self._emb_flags), self._stream())

    def _emb_moved(self, n_old: int, loader_version) -> None:
        """After a call that changed cfg.num_nodes, the row capacity or the loader's version without changing what an
        old row embeds to (grow_nodes, reserve_nodes, compact_events): the table and the planes move to the new
        capacity and plane stride, old rows keep their bits and their flags, new rows are stale (their embedding is
        not zero: the skip path and the biases act on a zero memory row), and the table's record of the loader
        version follows if it was current."""
        ver = self._emb_ver
        if ver is not None and ver[1] == loader_version:
            self._emb_ver = (ver[0], getattr(self.loader, "version", None))
        if self._emb_tab is None:
            return
        n, cap = int(self.cfg.num_nodes), max(self.node_capacity, int(self.cfg.num_nodes))
        if n == n_old and cap <= self._emb_tab.shape[0]:
            return
        tab, flags = self._emb_tab, self._emb_flags
        if cap > tab.shape[0]:
            self._emb_alloc(cap)
            self._emb_tab[:n_old].copy_(tab[:n_old])
        if n != n_old or flags is not self._emb_flags:
            # (D1 / D2 are zero between calls: only T carries flags across)
            t_old = flags[:n_old].clone()
            self._emb_flags.zero_()
            self._emb_flags[:n_old].copy_(t_old)
            self._emb_flags[n_old:n].fill_(1)

    def invalidate_embeddings(self) -> None:
        """Mark every row of the embedding table stale: for callers that write parameters, memory, last_update or the
        ring directly (a raw tensor write the engine cannot see; model.load_state_dict / load_reference_state and the
        loader's own calls are seen)."""
        self._emb_all = True

    @torch.no_grad()
    def refresh_embeddings(self) -> torch.Tensor:
        """Make the embedding table current and return the ids of the rows it recomputed (ascending int64, on the
        device): tgnx_embtab_expand and tgnx_embtab_list turn the touched endpoints into the stale list, one host read
        takes its length (as embed()'s validation reads the host), and tgnx_tgn_embed_into embeds the list in chunks
        of embed_capacity() straight into the table.  Nothing stale: no embed launch, an empty tensor.  Everything
        stale (after enable / invalidate_embeddings, a train step, flush, reset_state, a loaded stream state or
        parameters, a replayed eval pass): the list is arange(N), without the list kernels or the host read.
        The list is ascending and run-to-run identical, so a refresh is reproducible bit for bit; rows embedded in
        one chunk share GEMM calls, so the bits of a row may differ from embed()'s of another node set within its
        tolerance.  Read-only on the stream state as embed() is.  Nothing is flushed (see embed())."""
        if self._emb_tab is None:
            raise RuntimeError("refresh_embeddings: no embedding table (enable_embedding_table() first)")
        self._settle()
        N, cap = int(self.cfg.num_nodes), self.embed_capacity()
        if cap <= 0:
            raise RuntimeError(f"tgnx_tgn_embed_max_nodes: {_lib.lib().tgnx_last_error().decode()}")
        ver = (getattr(self.model, "_param_version", None), getattr(self.loader, "version", None))
        if ver != self._emb_ver:
            self._emb_all, self._emb_ver = True, ver
        b = self._buffers(0)
        if self._emb_all:
            self._emb_flags.zero_()
            ids = torch.arange(N, device=self.dev)
        else:
            _lib.call("tgnx_embtab_expand", ctypes.byref(self.cfg), ctypes.byref(b), _p(self._emb_flags), self._stream())
            _lib.call("tgnx_embtab_list", _p(self._emb_flags), N, int(self.cfg.layers), _p(self._emb_ids),
                      _p(self._emb_cnt), _p(self._emb_ws), self._emb_ws.numel(), self._stream())
            ids = self._emb_ids[:int(self._emb_cnt.item())].clone()
        n = ids.numel()
        self._emb_all = True    # (until the rows are written and checked)
        for a in range(0, n, cap):
            _lib.call("tgnx_tgn_embed_into", ctypes.byref(self.cfg), ctypes.byref(b), ids.data_ptr() + a * 8,
                      min(cap, n - a), _p(self._emb_tab), self._stream())
        if n:
            self.check()
        self._emb_all = False
        return ids

    def embedding_table(self) -> torch.Tensor:
        """The [N, D] table of current embeddings, refreshed first (refresh_embeddings): row v is embed([v]) within its
        tolerance — the export for a downstream index.  A view of the engine's table, not a copy: the next state
        change (observe, an eval or train batch, flush, reset, a load, grow_nodes) invalidates it, and the next
        refresh rewrites its stale rows in place; clone() what must outlive that."""
        self.refresh_embeddings()
        return self._emb_tab[:int(self.cfg.num_nodes)]

    def _embed_lists(self, lists, cached: bool, what: str = "embed", full=None):
        """One [n_i, D] block of embeddings per id list.  Uncached: one embed() over the concatenation, the blocks its
        row ranges.  Cached: rows of the refreshed embedding table (index_select; the list `full`, which the caller
        knows to be every node in order, is the table itself: no gather), ids checked against [0, N) by one host read
        as embed() checks them."""
        if not cached:
            z = self.embed(torch.cat(lists))
            out, a = [], 0
            for x in lists:
                out.append(z[a:a + x.numel()])
                a += x.numel()
            return out
        if self._emb_tab is None:
            raise RuntimeError(f"{what}: cached=True needs the embedding table (enable_embedding_table() first)")
        N = int(self.cfg.num_nodes)
        ids = torch.cat([x for i, x in enumerate(lists) if i != full])     # (never empty: `full` is not the sources)
        if ids.numel() and bool(((ids < 0) | (ids >= N)).any()):
            raise ValueError(f"{what}: node ids must be in [0, {N})")
        tab = self.embedding_table()
        return [tab if i == full else tab.index_select(0, x) for i, x in enumerate(lists)]

    def _all_nodes(self, candidates) -> bool:
        """The default candidates of an engine without dst_nodes: every node, in order."""
        return candidates is None and self.dst_nodes is None

    @torch.no_grad()
    def embed(self, nodes, validate: bool = True) -> torch.Tensor:
        """Embeddings [n, D] of `nodes` (any integer sequence / tensor; duplicates allowed) at the current stream
        state, as an eval batch computes them before scoring: memory and last_update as stored, the ring sampled for
        the node set, GraphAttentionEmbedding (tgnx_tgn_embed).  Read-only: memory, stores, ring, parameters and the
        batch cursor are untouched (ctl[3], the generation stamp, advances by one per chunk), so eval and train go on
        as if it had not been called; like every non-train call it makes the next resident step prepare its batch
        again.  Nothing is flushed: after train steps call flush() first (as tgn_epoch.test does), or the stored
        messages of the last batches are not in the memory rows read here.  Node sets beyond embed_capacity() run in
        chunks.  validate: one host read checks the ids against [0, N) and raises ValueError; without it an id out
        of range gets a zero row.  embed_cached() reads the embedding table instead."""
        self._settle()
        nodes = torch.as_tensor(nodes).to(self.dev, torch.long).contiguous().view(-1)
        n, N = nodes.numel(), self.cfg.num_nodes
        if validate and n and bool(((nodes < 0) | (nodes >= N)).any()):
            raise ValueError(f"embed: node ids must be in [0, {N})")
        out = torch.empty(n, self.cfg.mem_dim, dtype=torch.float32, device=self.dev)
        cap = self.embed_capacity()
        if cap <= 0:
            raise RuntimeError(f"tgnx_tgn_embed_max_nodes: {_lib.lib().tgnx_last_error().decode()}")
        b = self._buffers(0)
        for a in range(0, n, cap):
            m = min(cap, n - a)
            _lib.call("tgnx_tgn_embed", ctypes.byref(self.cfg), ctypes.byref(b), nodes.data_ptr() + a * 8, m,
                      out.data_ptr() + a * self.cfg.mem_dim * 4, 0, self._stream())
        if n:
            self.check()
        return out

    @torch.no_grad()
    def embed_cached(self, nodes) -> torch.Tensor:
        """embed() from the embedding table (enable_embedding_table; refreshed first, ids always validated): equal to
        embed()'s rows within its tolerance, not bit for bit.  (embed(), recommend() and score() keep their
        signatures; *_cached are their cached=True forms.)"""
        return self._embed_lists([self._ids(nodes)], True)[0]

    def _ids(self, x) -> torch.Tensor:
        """Node ids (any integer sequence / tensor) as a flat contiguous int64 tensor on the device."""
        return torch.as_tensor(x).to(self.dev, torch.long).contiguous().view(-1)

    def _candidates(self, candidates) -> torch.Tensor:
        """The candidate node ids of a query: the caller's, else the engine's dst_nodes, else every node."""
        if candidates is None:
            candidates = self.dst_nodes if self.dst_nodes is not None else \
                torch.arange(self.cfg.num_nodes, device=self.dev)
        return self._ids(candidates)

    def _link_weights(self):
        """The model's link_pred parameters in the order the link operators take them."""
        lp = self.model.link_pred
        return (lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias, lp.lin_final.weight,
                lp.lin_final.bias)

    @staticmethod
    def _node_ids(idx, table):
        """Selected positions into `table` as node ids; the padding (-1) stays."""
        return torch.where(idx >= 0, table[idx.clamp(min=0)], idx) if table.numel() else idx

    @torch.no_grad()
    def recommend(self, src, k: int, candidates=None, return_scores: bool = False):
        """For every source node the k candidates the model ranks highest at the current stream state:
        (val [Q, k] sigmoid outputs, node_ids [Q, k][, logits [Q, C]]).  candidates: node ids (default: the engine's
        dst_nodes when it has them, else every node).  Sources and candidates are embedded with embed() (read-only,
        chunked), then scored over all pairs and selected in one fused kernel with the model's link_pred parameters
        (ops.link_topk: ranked by logit, equal logits by the candidate's position in `candidates`).  k beyond the
        candidate count pads with node id -1 and val 0.  recommend_cached() reads the embedding table instead."""
        return self._recommend(src, k, candidates, return_scores, False)

    @torch.no_grad()
    def recommend_cached(self, src, k: int, candidates=None, return_scores: bool = False):
        """recommend() whose embeddings are rows of the embedding table (enable_embedding_table; refreshed first, so
        only the rows stale since the last query are recomputed); when the candidates are every node in order the
        table itself is the candidate operand, with no gather.  Also recommend_filtered(..., cached=True)."""
        return self._recommend(src, k, candidates, return_scores, True)

    def _recommend(self, src, k, candidates, return_scores, cached):
        from . import ops
        cand, src = self._candidates(candidates), self._ids(src)
        zs, zc = self._embed_lists([src, cand], cached, "recommend", 1 if self._all_nodes(candidates) else None)
        out = ops.link_topk(zs, zc, *self._link_weights(), k, sigmoid=True, return_scores=return_scores)
        return (out[0], self._node_ids(out[1], cand)) + tuple(out[2:])

    def _ragged_ids(self, x, n_src, what):
        """(ptr [n_src + 1], node ids, longest segment) on the device from a (ptr, ids) tuple of tensors / arrays or a
        sequence of n_src sequences; the ids checked against [0, N) and the pointers for shape (host reads)."""
        from . import ops
        if not (isinstance(x, tuple) and len(x) == 2 and all(isinstance(a, (torch.Tensor, np.ndarray)) for a in x)):
            rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in x]
            if len(rows) != n_src:
                raise ValueError(f"{what}: {len(rows)} lists for {n_src} sources")
            ptr = np.zeros(n_src + 1, dtype=np.int64)
            np.cumsum([r.size for r in rows], out=ptr[1:])
            x = (ptr, np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64))
        ptr, ids, longest = ops._ragged(x, n_src, self.dev, what, True, need_sorted=False)
        N = self.cfg.num_nodes
        if ids.numel() and bool(((ids < 0) | (ids >= N)).any()):
            raise ValueError(f"{what}: node ids must be in [0, {N})")
        return ptr, ids, longest

    def _segments(self, ptr, nnz):
        """The source row of every entry of a ragged array."""
        q = torch.arange(ptr.numel() - 1, device=self.dev)
        return torch.repeat_interleave(q, ptr[1:] - ptr[:-1], output_size=nnz)

    def _exclusions(self, src, exclude_seen, exclude, history=None):
        """(ptr [Q + 1], keys) of the per-source exclusions, each segment ascending: the valid entries of the source's
        neighbour-ring row (e_id >= 0; reset_state leaves stale ids in `neighbors`), the caller's lists and, with
        history = (candidates, since), the candidates the pair history says the source has met (PairSet.select: one
        host read for the length).  Invalid ring slots become the key N, which no node carries.  Device ops only
        otherwise; None when nothing is excluded."""
        N, Q = self.cfg.num_nodes, src.numel()
        seg, key = [], []
        if history is not None:
            ptr, ids = self._pair_set("exclude_history=True").select(src, history[0], history[1])
            key.append(ids)
            seg.append(self._segments(ptr, ids.numel()))
        if exclude_seen:
            ld = self.loader
            rows = torch.where(ld.e_id[src] >= 0, ld.neighbors[src], torch.full_like(ld.neighbors[src], N))
            key.append(rows.reshape(-1))
            seg.append(torch.arange(Q, device=self.dev).repeat_interleave(rows.shape[1]))
        if exclude is not None:
            ptr, ids, _ = self._ragged_ids(exclude, Q, "recommend: exclude")
            key.append(ids)
            seg.append(self._segments(ptr, ids.numel()))
        if not key:
            return None
        comp = torch.sort(torch.cat(seg) * (N + 1) + torch.cat(key)).values        # by source, then by key
        ptr = torch.searchsorted(comp, torch.arange(Q + 1, device=self.dev) * (N + 1))
        return ptr, comp % (N + 1), comp

    @torch.no_grad()
    def recommend_filtered(self, src, k: int, candidates=None, return_scores: bool = False, *,
                           exclude_seen: bool = False, exclude_self: bool = False, exclude=None, per_source=None,
                           cached: bool = False, exclude_history: bool = False, history_since=None):
        """recommend() with per-source exclusions and per-source candidate lists; read-only in the same way.
        exclude_seen: leave out the nodes in the source's neighbour-ring row (its most recent interaction partners).
        exclude_self: leave out the source itself.  exclude: more node ids per source, a (ptr, node_ids) tuple of
        tensors / arrays or a sequence of sequences, one per source.  Exclusion is by node id, so every position of a
        duplicated candidate goes.  Returns recommend()'s tuple; the logits are unmasked.
        per_source (not with `candidates`): every source's own candidate list, in the same two forms.  The engine
        embeds src and the distinct listed nodes once and ranks each source over its list only
        (ops.link_topk(lists=...)): equal logits by the entry's place in the list; excluded entries are masked in a
        private copy.  Returns (val [Q, k], node_ids [Q, k][, logits [nnz]]), the logits aligned with the caller's
        entries and NaN at an excluded one.  cached: the embeddings are rows of the embedding
        table (recommend_cached()).
        exclude_history (enable_pair_history() first, RuntimeError otherwise): leave out every candidate the source
        has ever interacted with as a source — the whole recorded history, not the ring's last `ring` partners;
        history_since: only pairs whose last interaction is at or after this stamp (a float, or one per source).  The
        met candidates come from PairSet.select and are merged with the other exclusions; a per_source list is
        filtered with PairSet.contains over its entries."""
        from . import ops
        src = self._ids(src)
        Q, N = src.numel(), self.cfg.num_nodes
        if Q and bool(((src < 0) | (src >= N)).any()):
            raise ValueError(f"recommend: node ids must be in [0, {N})")
        w = self._link_weights()
        ps = self._pair_set("exclude_history=True") if exclude_history else None
        # (the candidates are needed ahead of the exclusions only by the history's select)
        cand = self._candidates(candidates) if ps is not None and per_source is None else None
        ex = self._exclusions(src, exclude_seen, exclude, (cand, history_since) if cand is not None else None)
        if per_source is not None:
            if candidates is not None:
                raise ValueError("recommend: per_source and candidates are mutually exclusive")
            ptr, ids, longest = self._ragged_ids(per_source, Q, "recommend: per_source")
            uniq, pos = torch.unique(ids, return_inverse=True)
            zs, zu = self._embed_lists([src, uniq], cached, "recommend")
            seg = self._segments(ptr, ids.numel())
            pos = pos.clone()
            if exclude_self:
                pos[ids == src[seg]] = -1
            if ex is not None and ex[2].numel():
                comp = seg * (N + 1) + ids
                at = torch.searchsorted(ex[2], comp).clamp(max=ex[2].numel() - 1)
                pos[ex[2][at] == comp] = -1
            if ps is not None and ids.numel():
                since = history_since
                if torch.is_tensor(since) or isinstance(since, np.ndarray):
                    since = torch.as_tensor(since).to(self.dev, torch.float32).view(-1)[seg]
                pos[ps.contains(src[seg], ids, since)] = -1
            out = ops.link_topk(zs, zu, *w, k, sigmoid=True, return_scores=return_scores, lists=(ptr, pos),
                                validate=False, max_len=longest)
            return (out[0], self._node_ids(out[1], uniq)) + tuple(out[3:])
        if ex is None and not exclude_self:
            return self._recommend(src, k, candidates, return_scores, cached)
        if cand is None:
            cand = self._candidates(candidates)
        zs, zc = self._embed_lists([src, cand], cached, "recommend", 1 if self._all_nodes(candidates) else None)
        out = ops.link_topk(zs, zc, *w, k, sigmoid=True, return_scores=return_scores, cand_key=cand,
                            src_key=src if exclude_self else None, exclude=None if ex is None else ex[:2],
                            validate=False)
        return (out[0], self._node_ids(out[1], cand)) + tuple(out[2:])

    @torch.no_grad()
    def score(self, src, dst) -> torch.Tensor:
        """The model's link probability [n] for the explicit pairs (src[i], dst[i]) at the current stream state:
        embed() of both lists, then the LinkPredictor operator.  Read-only as embed() is.  score_cached() reads the
        embedding table instead."""
        return self._score(src, dst, False)

    @torch.no_grad()
    def score_cached(self, src, dst) -> torch.Tensor:
        """score() over rows of the embedding table (enable_embedding_table; refreshed first) instead of embed():
        what cached=True is to the other queries (score()'s signature is fixed at (src, dst))."""
        return self._score(src, dst, True)

    def _score(self, src, dst, cached: bool) -> torch.Tensor:
        from . import ops
        src, dst = self._ids(src), self._ids(dst)
        if src.numel() != dst.numel():
            raise ValueError(f"score: {src.numel()} sources for {dst.numel()} destinations")
        n = src.numel()
        zs, zd = self._embed_lists([src, dst], cached, "score")
        if n == 0:
            return zs.new_empty(0)
        return ops.link_predictor(zs.contiguous(), zd.contiguous(), *self._link_weights(), sigmoid=True).view(-1)

    # ------------------------------------------------------------------ why a score is what it is
    def _explain_nodes(self, nodes, mode: int, loo: bool, validate: bool, what: str) -> dict:
        """tgnx_tgn_explain over a node list, in chunks of embed_capacity(): z [n, D], count [n] int32, event /
        neighbour [n, K] int64, alpha [n, K, 2] and (loo) loo_z [n, K, D]."""
        self._settle()
        nodes = self._ids(nodes)
        n, N, K, D = nodes.numel(), self.cfg.num_nodes, self.cfg.ring, self.cfg.mem_dim
        if validate and n and bool(((nodes < 0) | (nodes >= N)).any()):
            raise ValueError(f"{what}: node ids must be in [0, {N})")
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = dict(z=torch.empty(n, D, **f32), count=torch.empty(n, dtype=torch.int32, device=self.dev),
                   event=torch.empty(n, K, dtype=torch.long, device=self.dev),
                   neighbour=torch.empty(n, K, dtype=torch.long, device=self.dev), alpha=torch.empty(n, K, 2, **f32))
        if loo:
            out["loo_z"] = torch.empty(n, K, D, **f32)
        cap = self.embed_capacity()
        if cap <= 0:
            raise RuntimeError(f"tgnx_tgn_embed_max_nodes: {_lib.lib().tgnx_last_error().decode()}")
        bad = torch.zeros(1, dtype=torch.long, device=self.dev)
        b = self._buffers(0)
        at = lambda t, a: t.data_ptr() + a * (t.numel() // max(n, 1)) * t.element_size()  # noqa: E731
        for a in range(0, n, cap):
            _lib.call("tgnx_tgn_explain", ctypes.byref(self.cfg), ctypes.byref(b), nodes.data_ptr() + a * 8,
                      min(cap, n - a), mode, at(out["z"], a), at(out["count"], a), at(out["event"], a),
                      at(out["neighbour"], a), at(out["alpha"], a), at(out["loo_z"], a) if loo else 0, _p(bad),
                      self._stream())
        if n:
            self.check()
        out["n_invalid"] = bad
        return out

    @torch.no_grad()
    def attention(self, nodes, validate: bool = True) -> dict:
        """What each node's embedding attends over at the current stream state: a dict with, per listed node, `count`
        [n] (the valid slots of its ring row), `neighbour` and `event` [n, K] (the slot's neighbour node and event row,
        in the sampler's order, -1 past count), `t` [n, K] (the event table's time of the slot, 0 past count), `alpha`
        [n, K, 2] (the eval-mode attention weight per head of the node's own TransformerConv softmax, 0 past count;
        at layers = 2 the root level's, conv2) and `z` [n, D], bit for bit embed()'s rows.  Read-only and chunked as
        embed() is (tgnx_tgn_explain without the leave-one-out rows).  validate: as embed(); without it an id out of
        range gets zero rows, count 0 and -1 slots, and is counted in `n_invalid` [1]."""
        o = self._explain_nodes(nodes, 0, False, validate, "attention")
        o["t"] = self._slot_times(o["event"])
        return o

    def _slot_times(self, event) -> torch.Tensor:
        """The event table's time of each slot's event row; 0 where the slot is padding (-1)."""
        return torch.where(event >= 0, self._tab[2][event.clamp(min=0)], torch.zeros((), device=self.dev))

    @torch.no_grad()
    def explain(self, src, dst, by: str = "slot") -> dict:
        """Which past interaction moved the link score of each pair (src[i], dst[i]), and by how much.  A node's
        embedding is its memory row plus one attention over the at most `ring` interactions of its ring row, so the
        effect of an interaction is exact: the same forward with that slot absent (tgnx_tgn_explain recomputes the
        softmax over the remaining slots; ops.link_loo scores every pair with one side's embedding replaced).
        Returns a dict: `logit`, `prob` [P]; `src_effect`, `dst_effect` [P, K] = logit - the logit without S_j
        (positive: the interaction raised the score; 0 past the node's count), where S_j is slot j (by="slot") or every
        slot naming slot j's neighbour (by="neighbour": repeat interactions removed together; `src_lead` / `dst_lead`
        [P, K] then mark the first slot of each neighbour group, the others repeat its effect); and per side
        `*_neighbour`, `*_event` [P, K] (-1 past count), `*_t`, `*_alpha` (mean over heads) [P, K], `*_count` [P].
        unique(src ∪ dst) is embedded once (in chunks beyond embed_capacity()): `nodes` [n] are those ids, `z` [n, D]
        (embed()'s rows, bit for bit) and `loo_z` [n, K, D] their embeddings and leave-one-out embeddings, and
        `src_row` / `dst_row` [P] each pair's rows among them.  Read-only as embed() is.  Built for
        the 1-hop embedding on one device: layers = 2 (removing an edge also changes the node's own hop-1 row) and a
        data-parallel engine raise NotImplementedError; attention() works at 2 hops."""
        from . import ops
        src, dst = self._ids(src), self._ids(dst)
        mode = check_explain_args(by, src.numel(), dst.numel(), 2 if self.cfg.layers == 2 else 1, self.world)
        N, P = self.cfg.num_nodes, src.numel()
        if P and bool(((src < 0) | (src >= N) | (dst < 0) | (dst >= N)).any()):
            raise ValueError(f"explain: node ids must be in [0, {N})")
        uniq, inv = torch.unique(torch.cat([src, dst]), return_inverse=True)
        o = self._explain_nodes(uniq, mode, True, False, "explain")
        rows = (inv[:P].contiguous(), inv[P:].contiguous())
        base, sl, dl, _ = ops.link_loo(o["z"], o["loo_z"], o["count"], rows[0], rows[1], *self._link_weights())
        ev = o["event"]
        t = self._slot_times(ev)
        alpha = o["alpha"].mean(-1)
        out = dict(logit=base, prob=torch.sigmoid(base), src_effect=base.view(-1, 1) - sl,
                   dst_effect=base.view(-1, 1) - dl, nodes=uniq, z=o["z"], loo_z=o["loo_z"], src_row=rows[0],
                   dst_row=rows[1])
        nb = o["neighbour"]
        for side, r in zip(("src", "dst"), rows):
            out[f"{side}_neighbour"], out[f"{side}_event"], out[f"{side}_t"] = nb[r], ev[r], t[r]
            out[f"{side}_alpha"], out[f"{side}_count"] = alpha[r], o["count"][r]
        if mode == 1:  # first slot of each neighbour group: no earlier slot of the row names the same neighbour
            K = nb.size(1)
            same = (nb.unsqueeze(2) == nb.unsqueeze(1)) & torch.ones(K, K, dtype=torch.bool, device=self.dev).tril(-1)
            lead = (nb >= 0) & ~same.any(2)
            out["src_lead"], out["dst_lead"] = lead[rows[0]], lead[rows[1]]
        return out

    @torch.no_grad()
    def rank(self, src, dst, candidates=None, return_scores: bool = False, *, exclude_seen: bool = False,
             exclude_self: bool = False, exclude=None, cached: bool = False, exclude_history: bool = False,
             history_since=None):
        """Where the model places the destination that happened: for every pair (src[i], dst[i]) the rank of dst[i]
        among the candidates recommend() would choose from (default: the same), at the current stream state and
        with recommend_filtered()'s exclusions (the "filtered" setting: the true destination itself is never
        excluded, and its own node never competes with it, wherever it occurs among the candidates).  Returns
        (rank [Q] float64 = 1 + gt + eq / 2, gt, eq, n [Q] int64, prob [Q][, logits [Q, C] unmasked]): gt / eq
        candidates scored above / equal to the destination, n compared, prob the destination's link probability.
        A destination outside `candidates` is ranked against all of them.  src, the candidates and dst are embedded
        once with embed(); the counts come from one fused pass (ops.link_rank), no [Q, C] logits unless asked for.
        Read-only as recommend() is.  cached: src and the candidate + destination rows are gathered from the embedding
        table (enable_embedding_table; refreshed first).  exclude_history / history_since: recommend_filtered()'s —
        the candidates the pair history says the source has met do not compete (the true destination still does)."""
        from . import ops
        src, dst = self._ids(src), self._ids(dst)
        Q, N = src.numel(), self.cfg.num_nodes
        if dst.numel() != Q:
            raise ValueError(f"rank: {Q} sources for {dst.numel()} destinations")
        if Q and bool(((src < 0) | (src >= N) | (dst < 0) | (dst >= N)).any()):
            raise ValueError(f"rank: node ids must be in [0, {N})")
        cand = self._candidates(candidates)
        C = cand.numel()
        ex = self._exclusions(src, exclude_seen, exclude, (cand, history_since) if exclude_history else None)
        if cached:
            zs, zc = self._embed_lists([src, torch.cat([cand, dst])], True, "rank")
        else:
            z = self.embed(torch.cat([src, cand, dst]))
            zs, zc = z[:Q], z[Q:]
        w = self._link_weights()
        rank, gt, eq, n, tlogit = ops.link_rank(
            zs, zc, *w, C + torch.arange(Q, device=self.dev), n_count=C, cand_key=torch.cat([cand, dst]),
            src_key=src if exclude_self else None, exclude=None if ex is None else ex[:2], validate=False)
        out = (rank, gt, eq, n, torch.sigmoid(tlogit))
        if return_scores:  # (over the same C + Q rows: the operands, and so the bits, of the counted logits)
            out += (ops.link_topk(zs, zc, *w, 1, sigmoid=False, return_scores=True)[2][:, :C].contiguous(),)
        return out

    def rank_events(self, start: int, B: int, candidates=None, *, exclude_seen: bool = False,
                    exclude_self: bool = False, exclude=None, cached: bool = False, exclude_history: bool = False,
                    history_since=None):
        """One prequential step over resident rows [start, start + B): rank() of src[e] -> dst[e] at the state before
        them, then observe(start, B).  Returns rank()'s tuple.  cached: rank(cached=True) — each step then embeds only
        the rows the previous step's batch made stale."""
        start, B = int(start), int(B)
        check_observe_args(start, B, self.cfg.max_batch, self.num_events, self.world)
        out = self.rank(self._tab[0][start:start + B], self._tab[1][start:start + B], candidates,
                        exclude_seen=exclude_seen, exclude_self=exclude_self, exclude=exclude, cached=cached,
                        exclude_history=exclude_history, history_since=history_since)
        self.observe(start, B)
        return out

    @torch.no_grad()
    def similar(self, nodes, k: int, candidates=None, *, metric: str = "cosine", exclude_self: bool = True,
                exclude_seen: bool = False, exclude=None, cached: bool = False, return_scores: bool = False):
        """Which nodes are like these: for every node of `nodes` its k nearest neighbours in embedding space at the
        current stream state, (score [Q, k], node_ids [Q, k][, scores [Q, C] unmasked]).  metric: "cosine" (default;
        a node with a zero embedding scores 0) or "dot".  candidates: node ids (default: every node [0, N) in order,
        whatever dst_nodes is — similarity is not restricted to destinations).  The link predictor takes no part:
        queries and candidates are embedded with embed() (read-only, chunked), then all pairs are scored on the f32
        MFMA and selected in the same kernel (ops.embed_knn: larger score first, equal scores by the candidate's
        position in `candidates`).  exclude_self (default True: under cosine a node is its own nearest neighbour)
        leaves the query node out, exclude_seen the nodes in its neighbour-ring row, exclude more node ids per query
        (recommend_filtered()'s forms); exclusion is by node id, so every position of a duplicated candidate goes.
        k beyond the candidates left pads with node id -1 and score -inf.  cached: the embeddings are rows of the
        embedding table (enable_embedding_table; refreshed first), and with the default candidates the table itself
        is the candidate operand, with no gather.  Read-only as recommend() is.  One device only.  (To leave out what
        the pair history says a query node has met, pass exclude=history_exclusions(nodes, candidates).)"""
        from . import ops
        if self.world > 1:
            raise ValueError("similar: one device only (world > 1 is not built)")
        ops.knn_metric(metric)
        k = ops.knn_k(k)
        nodes = self._ids(nodes)
        every = candidates is None
        cand = torch.arange(int(self.cfg.num_nodes), device=self.dev) if every else self._ids(candidates)
        # (embed() / the table path check every id against [0, N) with one host read, before the ring rows are read)
        zq, zc = self._embed_lists([nodes, cand], cached, "similar", 1 if every else None)
        ex = self._exclusions(nodes, exclude_seen, exclude)
        out = ops.embed_knn(zq, zc, k, metric=metric, return_scores=return_scores, cand_key=None if every else cand,
                            q_key=nodes if exclude_self else None, exclude=None if ex is None else ex[:2],
                            validate=False)
        return (out[0], self._node_ids(out[1], cand)) + tuple(out[2:])

    # ------------------------------------------------------------------ the live pair history
    def enable_pair_history(self, capacity=None) -> None:
        """Keep a live index of the (source, destination) pairs the stream has shown (off by default): a
        tgnx.pairset.PairSet on the device that every observe() / eval_batch() — and so observe_range, observe_events
        and rank_events — records its batch into with one more launch (tgnx_pairset_insert) after the step.  It holds
        counts and first / last stamps, no event rows, so compact_events() leaves it valid; grow_nodes only moves its
        id bound; forget_nodes erases the pairs that name a forgotten node; reset_state() empties it.  The resident
        eval pass and the train steps take their rows from a device cursor and do not record: record_pairs(lo, hi)
        does it for them.  capacity: initial slots (default and minimum: next_pow2(8 * max_batch), so a batch is one
        launch); it doubles by PairSet's rule, which reads the host once per capacity / 8 recorded events at most.
        Enabling twice keeps the history.  load_stream_state() does not touch it: pair_history_state() /
        load_pair_history_state() are its checkpoint (the drop-in save_stream / load_stream carry both).  One device
        only (ValueError at world > 1 / dp)."""
        from . import pairset
        if self.world > 1 or self.dp:
            raise ValueError("enable_pair_history: one device only (world > 1 is not built)")
        if self._pairs is None:
            cap = pairset.min_capacity(self.cfg.max_batch)
            if capacity is not None:
                cap = max(cap, pairset.check_capacity(capacity))
            self._pairs = pairset.PairSet(int(self.cfg.num_nodes), cap, device=self.dev)

    def disable_pair_history(self) -> None:
        """Free the history; every call issues exactly the launches it issues without the feature."""
        self._pairs = None

    def _pair_set(self, what: str):
        """The PairSet with its id bound at cfg.num_nodes, or RuntimeError naming enable_pair_history()."""
        ps = self._pairs
        if ps is None:
            raise RuntimeError(f"{what} needs the pair history: call enable_pair_history() first")
        if ps.num_nodes != int(self.cfg.num_nodes):
            ps.set_num_nodes(int(self.cfg.num_nodes))
        return ps

    def _pairs_touch(self, start: int, B: int) -> None:
        """Record event rows [start, start + B) in the pair history (nothing to do while it is off)."""
        if self._pairs is None or B <= 0:
            return
        tab = self._tab
        self._pair_set("record").insert_ptr(tab[0].data_ptr() + start * 8, tab[1].data_ptr() + start * 8,
                                            tab[2].data_ptr() + start * 4, B)

    def record_pairs(self, lo: int, hi: int) -> None:
        """Record resident rows [lo, hi) in the pair history without touching the stream state: for callers who
        trained or validated over them with the resident passes, which do not record."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.num_events:
            raise ValueError(f"record_pairs: rows [{lo}, {hi}) outside the event table ({self.num_events} events)")
        self._pair_set("record_pairs")
        self._pairs_touch(lo, hi - lo)

    def clear_pair_history(self) -> None:
        """Empty the pair history (its capacity stays)."""
        self._pair_set("clear_pair_history").clear()

    def seen(self, src, dst, since=None) -> torch.Tensor:
        """bool[n] on the device: has src[i] ever interacted with dst[i] (as source and destination, in the recorded
        batches) — with `since` (a float or one per query), at or after that stamp.  No host read."""
        return self._pair_set("seen").contains(src, dst, since)

    def pair_stats(self, src, dst):
        """(count int64[n], t_first float32[n], t_last float32[n]) of the pairs: 0 / +inf / -inf for one never seen."""
        return self._pair_set("pair_stats").lookup(src, dst)[1:]

    def history_exclusions(self, src, candidates=None, since=None):
        """(ptr int64[Q + 1], node ids) on the device: for every source the candidates (default: recommend()'s) the
        pair history says it has met (at or after `since`), in candidate order — PairSet.select, the list that
        exclude_history=True merges, in the form every query takes as exclude=.  One host read."""
        return self._pair_set("history_exclusions").select(self._ids(src), self._candidates(candidates), since)

    def pair_history_state(self) -> dict:
        """PairSet.state() of the history: the pairs sorted by key with counts and stamps (a checkpoint)."""
        return self._pair_set("pair_history_state").state()

    def load_pair_history_state(self, state: dict) -> None:
        """Replace the history by a pair_history_state() dict's (enabled here if it is not)."""
        self.enable_pair_history()
        self._pair_set("load_pair_history_state").load_state(state)

    # ------------------------------------------------------------------ hist_rnd evaluation negatives
    def pair_history(self):
        """The tgnx.tgb_negs.PairHistory over the resident event table: each source's distinct destinations and the
        first row of every pair.  Built on first use, rebuilt when num_events changed (append_events), dropped with the
        bindings by compact_events, forget_nodes and load_stream_state (they renumber or rewrite the rows)."""
        from .tgb_negs import PairHistory
        idx = self.__dict__.get("_pair_hist")
        if idx is None or idx.num_rows != self.num_events or idx.num_nodes != int(self.cfg.num_nodes):
            idx = PairHistory.build(self.src, self.dst, int(self.cfg.num_nodes))
            self._pair_hist = idx
        return idx

    def eval_negatives(self, lo: int, hi: int, k: int, *, hist_ratio: float = 0.5, hist_hi=None, seed: int = 0,
                       max_draws: int = 0) -> torch.Tensor:
        """TGB-style hist_rnd negatives for rows [lo, hi) of the resident table (tgnx.tgb_negs.tgb_negatives on the
        resident src / dst / t, the engine's dst_nodes as the pool, pair_history() as the index): int64 [hi - lo, k] on
        the device, the table bind_eval_resident takes.  The resident t is float32: a stream whose timestamps float32
        merges should generate from its float64 times (pyg_epoch_utils.tgb_negatives does).  World 1 only."""
        from .tgb_negs import tgb_negatives
        if self.world != 1:
            raise ValueError("eval_negatives: one device only (world 1)")
        pool = None if self.dst_nodes is None else torch.unique(self.dst_nodes)
        return tgb_negatives(self.src, self.dst, self.t, lo, hi, k, hist_ratio=hist_ratio, hist_hi=hist_hi, pool=pool,
                             seed=seed, index=self.pair_history(), max_draws=max_draws)

    # ------------------------------------------------------------------ resident eval pass
    def bind_eval_resident(self, split_lo: int, split_hi: int, batch: int, negs):
        """A validation / test pass over events [split_lo, split_hi) in batches of `batch`, resident on the device:
        negs ([split_hi - split_lo, Kn] integers; row e - split_lo = event e's negatives) is moved to the device once
        and kept alive here, the batch cursor lives in the control block (ctl[18], TGNX_CTL_EVAL_NB) and the
        per-event reciprocal ranks stay in eval_rr() until eval_mrr() reads them.  Drops the eval graphs of an
        earlier binding; the train binding and its graphs are untouched (unless Kn grows the workspace)."""
        lo, hi, batch = int(split_lo), int(split_hi), int(batch)
        negs = torch.as_tensor(negs)
        if negs.dim() != 2 or negs.shape[0] != hi - lo or negs.shape[1] < 1 or negs.dtype.is_floating_point \
                or negs.dtype == torch.bool:
            raise ValueError(f"bind_eval_resident: negs must be an integer [split_hi - split_lo, Kn] = [{hi - lo}, Kn] "
                             f"table, got {tuple(negs.shape)} {negs.dtype}")
        if not (0 <= lo <= hi <= self.src.numel()) or not (0 < batch <= self.cfg.max_batch):
            raise ValueError(f"bind_eval_resident: split [{lo}, {hi}) batch {batch} outside the event table "
                             f"({self.src.numel()} events) / max_batch ({self.cfg.max_batch})")
        self._settle()
        Kn = int(negs.shape[1])
        self.ensure_neg(Kn)
        self._ev = (lo, hi, batch, Kn)
        self._ev_negs = negs.to(self.dev, torch.long).contiguous()
        self._ev_rr = torch.zeros(hi - lo, dtype=torch.float64, device=self.dev)
        self._rebind_eval()
        self.begin_eval()

    def _rebind_eval(self):
        """The eval binding's buffer block from the engine's current tensors; its captured graphs are dropped."""
        self._ev_graphs = None
        if self._ev is not None:
            self._ev_buf = self._buffers(_p(self._ev_negs))
            self._ev_buf_ref = ctypes.byref(self._ev_buf)

    def begin_eval(self):
        """Rewind the eval cursor to split_lo (the start of a pass).  Like every non-train call it settles a deferred
        data-parallel apply and makes the next train step prepare its batch again."""
        self._settle()
        self._emb_all = True
        self.ctl[18] = 0

    def _eval_step(self):
        if self._ev is None:
            raise RuntimeError("TgnEngine: no eval pass bound (bind_eval_resident)")
        lo, hi, batch, Kn = self._ev
        self._emb_all = True   # (the batch comes from the device cursor: the host does not see its rows)
        _lib.call("tgnx_tgn_eval_step_resident", ctypes.byref(self.cfg), self._ev_buf_ref, lo, hi, batch, Kn, self.dp_rank,
                  self.world, self.seed, ctypes.c_void_p(self._ev_rr.data_ptr()), self._stream())

    def eval_resident_step(self):
        """One eager eval batch at the cursor (a step past the end of the split is a no-op).  Returns the batch's
        (pos, neg [max_batch, Kn], rr) buffers; the first B rows are the batch's."""
        self._settle()
        self._eval_step()
        Kn = self._ev[3]
        return self.out_pos, self.out_neg[:self.cfg.max_batch * Kn].view(-1, Kn), self.mrr

    def capture_eval(self, group: int = 8):
        """One eval step as a HIP graph, and (group >= 2) `group` consecutive steps as one more, so that a pass pays
        one graph launch per `group` batches (replay_eval_n)."""
        self.finish()
        torch.cuda.synchronize(self.dev)
        saved = self.ctl.clone()
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            self._eval_step()
        gk = None
        if group >= 2:
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk):
                for _ in range(group):
                    self._eval_step()
        torch.cuda.synchronize(self.dev)
        self.ctl.copy_(saved)
        self._ev_graphs = (g1, int(group) if gk is not None else 0, gk)

    def replay_eval_n(self, n: int):
        """Exactly n eval steps from the cursor: whole captured groups while at least a group's worth remains, single
        replays for the rest."""
        if self._ev_graphs is None:
            raise RuntimeError("TgnEngine: no captured eval step (capture_eval after bind_eval_resident; a new binding or "
                               "a grown workspace drops it)")
        self._settle()
        self._emb_all = True
        g1, k, gk = self._ev_graphs
        done = 0
        while done < n:
            if gk is not None and n - done >= k:
                gk.replay()
                done += k
            else:
                g1.replay()
                done += 1

    def eval_rr(self) -> torch.Tensor:
        """float64 [split_hi - split_lo] on the device: event e's reciprocal rank at [e - split_lo]."""
        return self._ev_rr

    def eval_mrr(self) -> float:
        """The reference's validation number (epoch_utils.py: the mean of the per-batch `perf` list): the mean over
        the split's batches, the partial last one included, of each batch's mean reciprocal rank.  Formed on the
        device by the same reductions as the per-batch loop's, so the float is the same; one synchronisation."""
        lo, hi, batch, _ = self._ev
        perf = [self._ev_rr[a - lo:min(hi, a + batch) - lo].mean() for a in range(lo, hi, batch)]
        return float(torch.stack(perf).mean()) if perf else float("nan")

    # ------------------------------------------------------------------ resident (graph-capturable)
    def bind_resident(self, split_lo: int, split_hi: int, batch: int, dropout: bool = True):
        """Consecutive batches of `batch` events over [split_lo, split_hi), negatives drawn on the
        device; the batch cursor lives in the control block (no host arguments change per step)."""
        self.finish()
        self._group = None   # (a step group captured for a previous binding)
        self._rebind_eval()  # (and the eval pass's graphs: held apart from the train graphs, dropped with them)
        self._res = (int(split_lo), int(split_hi), int(batch))
        self._res_drop = 1 if dropout else 0
        self._prefetched = False
        self._release_plan_table()
        if self.use_plan_table:   # the split's ring-insert / store plans, built once for every batch
            nbytes = int(_lib.lib().tgnx_tgn_plan_table_bytes(ctypes.byref(self.cfg), *self._res))
            if nbytes == 0:
                raise RuntimeError(f"tgnx_tgn_plan_table_bytes: {_lib.lib().tgnx_last_error().decode()}")
            self.plan_table = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            _lib.call("tgnx_tgn_plan_table", ctypes.byref(self.cfg), ctypes.byref(self._buffers(0)), *self._res,
                      _p(self.plan_table), nbytes, self._stream())
        self._res_buf = self._buffers(_p(self.neg_train))
        L = _lib.lib()
        self._res_fused = self._fused()
        self._f = (L.tgnx_tgnn_advance, L.tgnx_tgn_train_step if self._res_fused else L.tgnx_tgn_train_fwd_bwd,
                   L.tgnx_tgn_train_update, L.tgnx_tgn_apply_rows_update)
        self._cfg_ref, self._buf_ref = ctypes.byref(self.cfg), ctypes.byref(self._res_buf)
        self._ctl_p = ctypes.c_void_p(self.ctl.data_ptr())

    def _release_plan_table(self):
        """Drop the bound split's plan table, and the library's record of it (tgnx_tgn_plan_table_release): the
        caching allocator may hand its address to another tensor."""
        if self.plan_table is not None and hasattr(_lib.lib(), "tgnx_tgn_plan_table_release"):
            torch.cuda.synchronize(self.dev)      # (no step still reading it)
            _lib.lib().tgnx_tgn_plan_table_release(ctypes.c_void_p(self.plan_table.data_ptr()))
        self.plan_table = None

    def __del__(self):
        try:
            if getattr(self, "plan_table", None) is not None:
                _lib.lib().tgnx_tgn_plan_table_release(ctypes.c_void_p(self.plan_table.data_ptr()))
        except Exception:
            pass

    def begin_epoch(self):
        """pyg_epoch_utils.py:11-16: memory reset_state + neighbor_loader reset_state; cursor to 0."""
        self.reset_state()
        self.ctl[10] = 0
        self._prefetched = False

    def _pipelined(self) -> bool:
        return self.pipeline and self.fold_cursor and (self._res_fused or self.dp)

    def _pp(self) -> bool:
        """Parity-set steps: world 1 with Adam fused (tgnx_tgn_train_step_pp), or data parallel
        (tgnx_tgn_train_fwd_bwd_pp: the previous step's exchanged rows + Adam at the head of the step); 1 or 2
        hops (TGNX_PP_2HOP=0 keeps 2 hops on the pipelined step: comment-shaped 0.2462 vs 0.2383 ms)."""
        if not (self.parity_sets and self._pipelined()):
            return False
        if self.model.layers == 2 and os.environ.get("TGNX_PP_2HOP", "1") == "0":
            return False
        return self._res_fused if not self.dp else True

    def _dp_pp(self) -> bool:
        return self.dp and self._pp()

    # the resident step's entry point, keyed as the library's StepMode names the mode: (parity sets, pipelined, Adam
    # fused, the caller scans the next batch) -> (symbol, whether it takes rank / world: the world-1-only forms do not)
    _ENTRY = {(True, True, False, False): ("tgnx_tgn_train_fwd_bwd_pp", True),
              (True, True, True, False): ("tgnx_tgn_train_step_pp", False),
              (False, True, True, False): ("tgnx_tgn_train_step_pipelined", False),
              (False, True, False, True): ("tgnx_tgn_train_fwd_bwd_split", True),
              (False, True, False, False): ("tgnx_tgn_train_fwd_bwd_pipelined", True),
              (False, False, True, False): ("tgnx_tgn_train_step_resident", True),
              (False, False, False, False): ("tgnx_tgn_train_fwd_bwd_resident", True)}

    def _pre(self, prefetched: bool = False, parity=None, apply=None):
        self._emb_all = True
        adv, fb = self._f[:2]
        lo, hi, batch = self._res
        st = self._stream()
        if self.fold_cursor:   # the batch cursor folded into the step's first launches
            pp, pipelined = self._pp(), self._pipelined()
            name, ranked = self._ENTRY[pp, pipelined, bool(self._res_fused), self._split()]
            args = [lo, hi, batch] + ([self.dp_rank, self.world] if ranked else []) + [self.seed, self._res_drop]
            if pipelined:
                args.append(1 if prefetched else 0)
            if pp:
                args.append(self._parity if parity is None else parity)
            if self._dp_pp():   # the previous step's exchanged rows + Adam at the head of this one
                ap = self._apply_pending if apply is None else apply
                args += [1 if ap else 0, ctypes.c_void_p(self.xgather.data_ptr()), ctypes.c_int64(self.xgather.shape[0])]
            rc = getattr(_lib.lib(), name)(self._cfg_ref, self._buf_ref, *args, st)
        else:
            rc = adv(self._ctl_p, 1, 0, 0, 0, lo, hi, batch, self.dp_rank, self.world, self.seed, 1, st)
            rc |= fb(self._cfg_ref, self._buf_ref, 1, self._res_drop, st)
        if rc:
            raise RuntimeError(f"tgnx TGN resident step failed: {_lib.lib().tgnx_last_error().decode()}")

    def _post(self):
        st = self._stream()
        rc = 0
        if self.dp:   # the exchanged rows and Adam, one launch
            rc |= self._f[3](self._cfg_ref, self._buf_ref, ctypes.c_void_p(self.xgather.data_ptr()),
                             ctypes.c_int64(self.xgather.shape[0]), st)
        elif not self._res_fused:   # fused step: Adam already applied
            rc |= self._f[2](self._cfg_ref, self._buf_ref, st)
        if rc:
            raise RuntimeError(f"tgnx TGN resident update failed: {_lib.lib().tgnx_last_error().decode()}")

    def _split(self) -> bool:
        return self.split_scan and self.dp and self._pipelined() and not self._res_fused and not self._pp()

    def _scan_next(self):
        """The next batch's scan (split pipelined steps): rides beside the exchange."""
        if self._split():
            lo, hi, batch = self._res
            _lib.call("tgnx_tgn_scan_next", self._cfg_ref, self._buf_ref, lo, hi, batch, self.dp_rank, self.world, self.seed,
                      self._stream())

    def _allreduce(self, between=None):
        """The exchange; `between` (the next batch's scan) runs on the compute stream while it is in flight."""
        if self.dp:
            if self.exchange is not None:
                work = self.exchange(self.comm, True)
                works = [] if work is None else [work]
            else:
                works = exchange_collectives(self.comm, self.model.grad_flat.numel(), self.dp_rank, self.world,
                                             self.exchange_mode, async_op=True)
            if between is not None:
                between()
            for w in works:
                w.wait()
        elif between is not None:
            between()

    def _prefetch_valid(self) -> bool:
        """The previous pipelined step's preparation of this batch still holds: no other engine call since
        (tracked by _prefetched) and no host-side change of the ring through the loader (its version)."""
        return self._prefetched and getattr(self.loader, "version", None) == self._prefetch_version

    def _mark_prefetched(self):
        self._prefetched = self._pipelined()
        self._prefetch_version = getattr(self.loader, "version", None)

    def resident_train_step(self):
        if self._dp_pp():   # [apply(k - 1) ‖ step k], then the exchange; its apply heads the next step
            self._pre(self._prefetch_valid(), apply=self._apply_pending)
            self._apply_pending = False
            self._allreduce()
            self._apply_pending = True
            self._mark_prefetched()
            self._parity ^= 1
            return
        self._pre(self._prefetch_valid())
        self._allreduce(self._scan_next)
        self._post()
        self._mark_prefetched()
        self._parity ^= 1 if self._pp() else 0

    def finish(self):
        """Apply a data-parallel parity-set step's exchange now (tgnx_tgn_apply_rows_update: the gathered
        memory rows and Adam) instead of at the head of the next step.  Every call that reads or rewrites the
        state runs this first; replays then take the graph without the apply."""
        if not self._apply_pending:
            return
        self._apply_pending = False  # (cleared whether or not the apply succeeds: a failed one is not retried)
        self._emb_all = True
        _lib.call("tgnx_tgn_apply_rows_update", self._cfg_ref, self._buf_ref, ctypes.c_void_p(self.xgather.data_ptr()),
                  ctypes.c_int64(self.xgather.shape[0]), self._stream())

    def capture_resident(self):
        """One resident step as HIP graph(s) (world > 1: the collectives stay eager between them)."""
        torch.cuda.synchronize(self.dev)
        saved = self.ctl.clone()
        if self._dp_pp():   # per parity, with and without the previous step's apply at its head; the collective stays eager
            gd = {}
            for par in (0, 1):
                for ap in (0, 1):
                    gd[par, ap] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gd[par, ap]):
                        self._pre(True, par, bool(ap))
            self._graphs = (gd, None, None)
        elif not self.dp and self._pp():   # one graph per parity, replayed alternately
            gp = (torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph())
            for par in (0, 1):
                with torch.cuda.graph(gp[par]):
                    self._pre(True, par)
            self._graphs = (gp, None, None)
        elif not self.dp:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):   # pipelined: the steady-state step (the previous step prefetched)
                self._pre(True)
                self._post()
            self._graphs = (g, None, None)
        else:
            g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):   # pipelined: the steady-state step (the previous step prefetched)
                self._pre(self._pipelined())
            gs = None
            if self._split():
                gs = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gs):
                    self._scan_next()
            with torch.cuda.graph(g2):
                self._post()
            self._graphs = (g1, g2, gs)
        torch.cuda.synchronize(self.dev)
        self.ctl.copy_(saved)

    def capture_group(self, k: int = 8):
        """World 1, parity-set steps: also capture k consecutive steps (parities 0, 1, 0, ...) as ONE HIP graph, so a
        run of steps pays one graph launch per k (replay_resident_n).  k even: the group starts and ends at parity 0."""
        if self.dp or not self._pp() or k < 2 or k % 2:
            self._group = None
            return False
        torch.cuda.synchronize(self.dev)
        saved = self.ctl.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for q in range(k):
                self._pre(True, q & 1)
        torch.cuda.synchronize(self.dev)
        self.ctl.copy_(saved)
        self._group = (k, g)
        return True

    def replay_resident_n(self, n: int):
        """n resident steps: whole captured k-step groups wherever the set parity and the prefetch allow, single
        replays (or the priming eager step) otherwise.  The same steps as n calls of replay_resident()."""
        grp = getattr(self, "_group", None)
        self._emb_all = True
        done = 0
        while done < n:
            if grp and n - done >= grp[0] and self._parity == 0 and self._prefetch_valid():
                grp[1].replay()
                self._mark_prefetched()
                done += grp[0]
            else:
                self.replay_resident()
                done += 1

    def replay_resident(self):
        self._emb_all = True
        g1, g2, gs = self._graphs
        if self._pipelined() and not self._prefetch_valid():
            self.resident_train_step()   # marks + scans this batch first (eager), prefetches the next
            return
        if isinstance(g1, dict):   # data-parallel parity graphs
            g1[self._parity, 1 if self._apply_pending else 0].replay()
            self._apply_pending = False
            self._allreduce()
            self._apply_pending = True
            self._parity ^= 1
            self._mark_prefetched()
            return
        if isinstance(g1, tuple):   # parity graphs
            g1[self._parity].replay()
            self._parity ^= 1
            self._mark_prefetched()
            return
        g1.replay()
        if g2 is not None:
            self._allreduce(gs.replay if gs is not None else None)
            g2.replay()
        self._mark_prefetched()

    def units(self):
        """(sum of sampled edges, sum of sampled nodes) since the last reset."""
        return int(self.ctl[13]), int(self.ctl[14])

    def loss_sum(self) -> float:
        self.finish()   # (the loss sum is accumulated by the Adam launch)
        return float(self.ctl[12:13].view(torch.float64).item())

    ERR_BITS = {4: "batch or sampled node / edge set beyond the workspace capacity",
                8: "more updated memory rows than the exchange slots hold (xcap)",
                16: "stale scan-output set: tgnx_tgn_train_step_pp / _fwd_bwd_pp called with the wrong parity, "
                    "or a prefetch that no longer holds",
                32: "edge sort beyond its LDS counters"}

    def check(self, settle: bool = True):
        """Raise on the step error flags (ctl[11]).  settle: first apply a deferred data-parallel exchange
        (finish()), so the state is current afterwards; False leaves it pending (tests that perform the
        exchange themselves after the step returned)."""
        if settle:
            self.finish()
        err = int(self.ctl[11].item())
        if err:
            why = "; ".join(m for b, m in self.ERR_BITS.items() if err & b) or "unknown"
            raise RuntimeError(f"tgnx TGN step error flags {err:#x}: {why}")


# config/TGN.yml memory section -> the PyG TGN's modules (TGL key names; TGN.yml:10-18)
MAIL_COMBINE = {"last": "last", "mean": "mean"}          # msg_agg.py LastAggregator / MeanAggregator
MEMORY_UPDATE = {"gru": "gru", "rnn": "rnn"}             # memory_module.py:70-78 memory_updater_cell


def model_options(gnn_param=None, memory_param=None, sample_param=None, train_param=None) -> dict:
    """TGNModel keywords from config/TGN.yml sections (utils.parse_config order).  gnn: `layer` -> layers
    (attention hops, 1 or 2); memory: `mail_combine` -> aggr, `memory_update` -> updater, `type` must be
    'node' (TGL's 'none' is a memory-less model, not the TGN path); sampling: `neighbor[0]` -> ring;
    train: `batch_size` -> max_batch.  When only gnn_param is given and it came from tgnx's parse_config
    (as in pyg-mem-tgn.py:36,49), the other sections of the same file are used."""
    from .data import config_of
    if gnn_param is not None and memory_param is None:
        got = config_of(gnn_param)
        if got is not None:
            sample_param = sample_param if sample_param is not None else got[0]
            memory_param = got[1]
            train_param = train_param if train_param is not None else got[3]
    out = {}
    if gnn_param is not None and "layer" in gnn_param:
        out["layers"] = int(gnn_param["layer"])
    if memory_param is not None:
        typ = memory_param.get("type", "node")
        if typ != "node":
            raise NotImplementedError(f"memory.type {typ!r}: only 'node' memory (TGNMemory) is the TGN path")
        mc = memory_param.get("mail_combine", "last")
        if mc not in MAIL_COMBINE:
            raise ValueError(f"memory.mail_combine must be 'last' or 'mean' (msg_agg.py), got {mc!r}")
        mu = memory_param.get("memory_update", "gru")
        if mu not in MEMORY_UPDATE:
            raise ValueError(f"memory.memory_update must be 'gru' or 'rnn' (memory_module.py:70-78), got {mu!r}")
        out["aggr"], out["updater"] = MAIL_COMBINE[mc], MEMORY_UPDATE[mu]
    if sample_param is not None and sample_param.get("neighbor"):
        out["ring"] = int(sample_param["neighbor"][0])
    if train_param is not None and "batch_size" in train_param:
        out["max_batch"] = int(train_param["batch_size"])
    return out


def getModel(feature_dim, hidden_dim, num_nodes, device, gnn_param=None, memory_param=None, num_events=None, **kw):
    """pyg_model_utils.py:10-36 with the call of pyg-mem-tgn.py:49 (`gnn_param=`; the reference's own
    getModel lacks it): hidden_dim is the memory / time / embedding width (gnn dim_out), and the config
    sections select the model (model_options: layer, mail_combine, memory_update, neighbor, batch_size).
    num_events (optional) pre-sizes the message-store arena; otherwise the engine sizes it when it binds
    the event table.  Explicit keywords win over the config: ring, max_batch, max_neg, aggr, dropout,
    layers, updater = 'gru' | 'rnn' (TGNMemory memory_updater_cell), memory = 'tgn' | 'dyrep'
    (DyRepMemory as the memory module, modules/memory_module.py:218-421; TGNModel)."""
    opts = model_options(gnn_param, memory_param)
    opts.update(kw)
    m = TGNModel(num_nodes, num_events, feature_dim, hidden_dim, device, **opts)
    return {"memory": m.memory, "gnn": m.gnn, "link_pred": m.link_pred, "model": m}


def getOptimizer(model, lr):
    return TgnAdam(model["model"], lr)
