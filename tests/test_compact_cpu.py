"""CPU checks of event-table compaction and the stream-state checkpoint: the library exports the three entry points
and their ctypes signatures restate the header's argument lists, the Python methods and drop-ins exist, the C calls
refuse bad arguments before any device call (the pointers handed in are host memory, as in test_observe_cpu.py), the
pure helpers — compact_events' argument check and capacity rule, the stream state's key list and its format /
fingerprint / shape check on hand-made dicts — hold without a device, and the numpy restatement of the live set the
GPU tests compare against gives the answer written out here for a six-event example."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from compact_ref import deref, live_rows
from conftest import ROOT

NAMES = {"tgnx_tgn_compact_ws_bytes": ("size_t", 2), "tgnx_tgn_compact_plan": ("int", 7),
         "tgnx_tgn_compact_apply": ("int", 14)}


def test_library_exports_and_binds_the_entry_points():
    from tgnx import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tgnx.h")).read(), flags=re.S)
    for name, (res, nargs) in NAMES.items():
        assert hasattr(L, name) and name in _lib.SIGNATURES
        m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m and m.group(1) == res
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (ctypes.c_size_t if res == "size_t" else ctypes.c_int)
        decl = [a.strip() for a in m.group(2).split(",")]
        assert len(decl) == len(args) == nargs, name
        for a, c in zip(decl, args):                       # pointers cross as void*, row counts as int64
            assert ("*" in a) == (c is _lib.P), (name, a)
            assert not a.startswith("int64_t ") or c is ctypes.c_int64, (name, a)
    assert os.path.exists(os.path.join(ROOT, "tgb-tgn-dgl_amd", "csrc", "tgnx_compact.hip"))


def test_python_surface_exists():
    import inspect

    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.tgn import TgnEngine
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(TgnEngine.compact_events) == ["self", "upto", "capacity"]
    assert all(p.default is None for p in list(inspect.signature(TgnEngine.compact_events).parameters.values())[1:])
    assert par(TgnEngine.stream_state) == ["self"] and par(TgnEngine.load_stream_state) == ["self", "state"]
    assert "upto" in TgnEngine.compact_events.__doc__ and "not observed" in TgnEngine.compact_events.__doc__
    assert par(tgn_epoch.compact) == ["model", "neighbor_loader", "upto", "capacity"]
    assert par(tgn_epoch.save_stream) == ["model", "neighbor_loader", "f"]
    assert par(tgn_epoch.load_stream)[:3] == ["model", "neighbor_loader", "f"]
    for name in ("compact", "save_stream", "load_stream"):
        assert getattr(pyg_epoch_utils, name) is getattr(tgn_epoch, name)


def _tgn_cfg(**kw):
    from tgnx.tgn import TgnConfig
    base = dict(num_nodes=300, num_events=600, ring=10, mem_dim=32, msg_dim=16, heads=2, max_batch=8, max_neg=1,
                aggr=0, dropout=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, layers=1, updater=0, emb_in_msg=0)
    base.update(kw)
    return TgnConfig(**base)


def test_c_calls_check_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers
    L = _lib.lib()
    cfg = _tgn_cfg()
    nb = int(L.tgnx_tgn_compact_ws_bytes(ctypes.byref(cfg), 600))
    # record + bitmap + word prefix + node prefix + workgroup sums, each padded to 256 bytes
    assert nb >= 64 + 2 * 4 * 19 + 4 * 300 and nb % 256 == 0 and nb < 1 << 14
    assert nb <= int(L.tgnx_tgn_compact_ws_bytes(ctypes.byref(cfg), 100_000)) < 100_000
    assert int(L.tgnx_tgn_compact_ws_bytes(ctypes.byref(cfg), 0)) > 0
    for bad in ((None, 600), (ctypes.byref(cfg), -1), (ctypes.byref(cfg), 1 << 30),
                (ctypes.byref(_tgn_cfg(num_nodes=0)), 600)):
        assert int(L.tgnx_tgn_compact_ws_bytes(*bad)) == 0
    keep = np.zeros(max(nb // 4, 256), dtype=np.float32)           # host memory: must never be touched
    p = ctypes.c_void_p(keep.ctypes.data)
    null = ctypes.c_void_p(0)

    def bufs(**zero):
        b = TgnBuffers()
        for f in ("ev_src", "ev_dst", "ev_t", "ev_msg", "nbr", "eid", "store", "ctl"):
            setattr(b, f, 0 if f in zero else p.value)
        return b

    def plan(cfg_ref=None, b=None, n=600, upto=600, ws=p, ws_bytes=nb):
        return L.tgnx_tgn_compact_plan(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                       ctypes.byref(bufs()) if b is None else b, n, upto, ws, ws_bytes, null)

    def apply(cfg_ref=None, b=None, n=600, cap=600, out=(p,) * 6, kept_len=600, ws=p, ws_bytes=nb):
        return L.tgnx_tgn_compact_apply(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                        ctypes.byref(bufs()) if b is None else b, n, cap, *out, kept_len, ws, ws_bytes,
                                        null)

    def failed(rc, code=-1):
        return rc == code and len(L.tgnx_last_error()) > 0

    for f in (plan, apply):
        assert failed(f(cfg_ref=null)) and failed(f(b=null))
        assert f.__name__.encode() in L.tgnx_last_error()
        for field in ("ctl", "nbr", "eid", "store"):
            assert failed(f(b=ctypes.byref(bufs(**{field: 1})))), field
        assert failed(f(ws=null)) and failed(f(ws_bytes=nb - 1)) and failed(f(ws=ctypes.c_void_p(p.value + 4)))
        assert failed(f(n=-1)) and failed(f(n=601))                        # beyond the capacity cfg.num_events
        assert failed(f(cfg_ref=ctypes.byref(_tgn_cfg(num_events=1 << 31)), n=1 << 30, ws_bytes=1 << 40), code=-3)
        for bad in (dict(num_nodes=0), dict(ring=0), dict(num_events=0)):
            assert failed(f(cfg_ref=ctypes.byref(_tgn_cfg(**bad)))), bad
    assert failed(plan(upto=-1)) and failed(plan(upto=601))
    for field in ("ev_src", "ev_dst", "ev_t", "ev_msg"):
        assert failed(apply(b=ctypes.byref(bufs(**{field: 1})))), field
    for i in range(6):
        assert failed(apply(out=tuple(null if j == i else p for j in range(6)))), i
    assert failed(apply(cap=0)) and failed(apply(kept_len=-1)) and failed(apply(cap=1 << 30))
    assert keep.sum() == 0


def test_check_compact_args():
    from tgnx.tgn import check_compact_args
    assert check_compact_args(600) == 600 and check_compact_args(600, None, None) == 600
    assert check_compact_args(600, 0) == 0 and check_compact_args(600, 599, 1) == 599 and check_compact_args(0) == 0
    for bad in ((600, 601), (600, -1), (0, 1)):
        with pytest.raises(ValueError, match="upto"):
            check_compact_args(*bad)
    for cap in (0, -5):
        with pytest.raises(ValueError, match="capacity"):
            check_compact_args(600, None, cap)
    with pytest.raises(ValueError, match="world"):
        check_compact_args(600, world=2)


def test_compact_capacity_is_the_grown_capacity_rule():
    from tgnx.tgn import compact_capacity, grown_capacity
    assert compact_capacity(0) == 1 and compact_capacity(1) == 2 and compact_capacity(2) == 3
    assert compact_capacity(255) == 382 and compact_capacity(487) == 730
    for n in (0, 1, 7, 100, 12345):
        cap = compact_capacity(n)
        assert cap == grown_capacity(n, n + 1) > n               # room for the next append
        assert grown_capacity(cap, n + 1) == cap                 # which therefore does not reallocate
    assert compact_capacity(255, 255) == 255 and compact_capacity(255, 4000) == 4000 and compact_capacity(0, 1) == 1
    for n, cap in ((255, 254), (1, 0), (0, 0)):
        with pytest.raises(ValueError, match="capacity"):
            compact_capacity(n, cap)
    with pytest.raises(ValueError):
        compact_capacity(-1)


def _state(N=3, K=2, D=4, d=5, n=6, **over):
    st = dict(format=1, num_nodes=N, ring=K, mem_dim=D, msg_dim=d, num_events=n,
              src=torch.zeros(n, dtype=torch.long), dst=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
              msg=torch.zeros(n, d), memory=torch.zeros(N, D), last_update=torch.zeros(N, dtype=torch.long),
              node_gen=torch.zeros(N, dtype=torch.int32), store_nodes=torch.zeros(N, 4, dtype=torch.long),
              store_arena=torch.zeros(2 * n, dtype=torch.long), neighbors=torch.zeros(N, K, dtype=torch.long),
              e_id=torch.zeros(N, K, dtype=torch.long), ring_t=torch.zeros(N, K), ctl=torch.zeros(24, dtype=torch.long))
    st.update(over)
    return st


def test_stream_state_keys_and_check():
    from tgnx.tgn import (STREAM_FINGERPRINT, STREAM_STATE_KEYS, STREAM_STATE_FORMAT, TgnConfig, check_stream_state,
                          stream_fingerprint)
    assert STREAM_STATE_FORMAT == 1 and STREAM_FINGERPRINT == ("num_nodes", "ring", "mem_dim", "msg_dim")
    assert STREAM_STATE_KEYS == ("format", "num_nodes", "ring", "mem_dim", "msg_dim", "num_events", "src", "dst", "t",
                                 "msg", "memory", "last_update", "node_gen", "store_nodes", "store_arena", "neighbors",
                                 "e_id", "ring_t", "ctl")
    assert tuple(_state()) == STREAM_STATE_KEYS
    fp = dict(num_nodes=3, ring=2, mem_dim=4, msg_dim=5)
    assert stream_fingerprint(TgnConfig(num_nodes=3, num_events=9, ring=2, mem_dim=4, msg_dim=5)) == fp
    assert check_stream_state(_state(), fp) == 6 and check_stream_state(_state(n=0), fp) == 0
    with pytest.raises(ValueError, match="format"):
        check_stream_state(_state(format=2), fp)
    with pytest.raises(ValueError, match="format"):
        check_stream_state({"src": 1}, fp)
    for k, v in (("ring", 10), ("num_nodes", 4), ("mem_dim", 8), ("msg_dim", 16)):
        with pytest.raises(ValueError, match="fingerprint"):
            check_stream_state(_state(), dict(fp, **{k: v}))
    st = _state()
    del st["store_arena"]
    with pytest.raises(ValueError, match="missing"):
        check_stream_state(st, fp)
    for k, v in (("msg", torch.zeros(6, 4)), ("src", torch.zeros(5, dtype=torch.long)),
                 ("store_arena", torch.zeros(6, dtype=torch.long)), ("e_id", torch.zeros(3, 3, dtype=torch.long)),
                 ("ctl", torch.zeros(8, dtype=torch.long)), ("memory", 3)):
        with pytest.raises(ValueError, match=k):
            check_stream_state(_state(**{k: v}), fp)
    with pytest.raises(ValueError, match="num_events"):
        check_stream_state(_state(num_events=-1), fp)


def _six_events():
    """Three nodes, ring 2 (second slot never filled: its e_id word is stale and must not count), batches of 2:
         batch 1   e0: 0 -> 1    e1: 2 -> 1        arena [0, 4)  = 0 | 0 1 | 1     (node 0 s, node 1 d, node 2 s)
         batch 2   e2: 0 -> 1    e3: 0 -> 1        arena [4, 8)  = 2 3 | 2 3
         batch 3   e4: 0 -> 1    e5: 0 -> 1        arena [8, 12) = 4 5 | 4 5
    with a ring that keeps one neighbour: node 0 and node 1 hold e5, node 2 holds e1.  Node 2 was last touched in
    batch 1, so its s run still names e1; the runs of nodes 0 and 1 were rewritten by batch 3."""
    nbr = np.array([[1, -1], [0, -1], [1, -1]])
    eid = np.array([[5, 0], [5, 0], [1, 0]])
    nodes = np.array([[8, 2, 0, 0], [0, 0, 10, 2], [3, 1, 0, 0]])
    arena = np.array([0, 0, 1, 1, 2, 3, 2, 3, 4, 5, 4, 5])
    return nbr, eid, nodes, arena


def test_live_set_restatement_on_six_events():
    nbr, eid, nodes, arena = _six_events()
    live, ring, stores = live_rows(nbr, eid, nodes, arena, 6)
    assert live.tolist() == [1, 4, 5] and live.dtype == np.int64
    assert ring == {1, 5} and stores == {1, 4, 5} and stores - ring == {4}        # e4 lives through the stores alone
    assert live_rows(nbr, eid, nodes, arena, 6, upto=3)[0].tolist() == [1, 3, 4, 5]
    assert live_rows(nbr, eid, nodes, arena, 6, upto=0)[0].tolist() == [0, 1, 2, 3, 4, 5]
    assert live_rows(nbr, eid, nodes, arena, 6, upto=6)[0].tolist() == [1, 4, 5]
    # the renumbering the kernels perform, done by hand: new id = rank among the live rows
    new = {1: 0, 4: 1, 5: 2}
    eid2 = np.array([[2, 0], [2, 0], [0, 0]])
    nodes2 = np.array([[0, 2, 0, 0], [0, 0, 2, 2], [4, 1, 0, 0]])                # node by node, s run then d run
    arena2 = np.array([new[4], new[5], new[4], new[5], new[1], 0])
    assert live_rows(nbr, eid2, nodes2, arena2, 3)[0].tolist() == [0, 1, 2]
    rng = np.random.default_rng(0)
    tab = dict(src=rng.integers(0, 3, 6), dst=rng.integers(0, 3, 6), t=rng.random(6).astype(np.float32),
               msg=rng.random((6, 5)).astype(np.float32))
    h0 = dict(nbr=nbr, eid=eid, rt=np.ones((3, 2), np.float32), nodes=nodes, arena=arena, **tab)
    h1 = dict(nbr=nbr, eid=eid2, rt=np.ones((3, 2), np.float32), nodes=nodes2, arena=arena2,
              **{k: v[live] for k, v in tab.items()})
    d0, d1 = deref(h0), deref(h1)
    assert sorted(d0) == sorted(d1) and all(np.array_equal(d0[k], d1[k]) for k in d0)
    assert d0["store_src"].shape[0] == 5 and d0["ring_src"].shape[0] == 3
