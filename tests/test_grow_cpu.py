"""CPU checks of node-space growth: the library exports the two entry points and their ctypes signatures restate the
header's argument lists, the Python methods and drop-ins exist with every earlier signature unchanged, the C calls
refuse bad arguments before any device call (the pointers handed in are host memory, as in test_compact_cpu.py), and
the pure helpers hold without a device: the capacity rule, the argument checks, the relaxed stream-state check beside
the strict one, and the pad reference the GPU tests compare against on a hand-made state."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from grow_ref import RESET_ROW, crop_state, is_reset_rows, pad_state, same_state
from test_compact_cpu import _state, _tgn_cfg

NAMES = {"tgnx_tgn_grow_nodes": ("int", 7), "tgnx_tgn_grow_store": ("int", 6)}


def test_header_declares_and_library_exports_the_entry_points():
    from tgnx import _lib
    raw = open(os.path.join(ROOT, "include", "tgnx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert re.search(r"}\s*tgnx_tgn_grow_out\s*;", hdr)
    decls = {}
    for name, (res, nargs) in NAMES.items():
        m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m and m.group(1) == res, name
        decls[name] = [a.strip() for a in m.group(2).split(",")]
        assert len(decls[name]) == nargs, name
        assert name in _lib.SIGNATURES
    assert os.path.exists(os.path.join(ROOT, "tgb-tgn-dgl_amd", "csrc", "tgnx_grow.hip"))
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtgnx.so is not built here")
    L = _lib.lib()
    for name, decl in decls.items():
        assert hasattr(L, name)
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is ctypes.c_int and len(args) == len(decl)
        for a, c in zip(decl, args):                       # pointers cross as void*, node counts as int64
            assert ("*" in a) == (c is _lib.P), (name, a)
            assert not a.startswith("int64_t ") or c is ctypes.c_int64, (name, a)


def test_grow_out_struct_matches_the_header():
    from tgnx.tgn import NODE_ROW_TENSORS, TgnBuffers, TgnGrowOut
    hdr = open(os.path.join(ROOT, "include", "tgnx.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*tgnx_tgn_grow_out;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = re.findall(r"\*\s*([a-z_]+)", body)
    assert fields == [f for f, _ in TgnGrowOut._fields_] and len(fields) == 8
    assert ctypes.sizeof(TgnGrowOut) == 8 * ctypes.sizeof(ctypes.c_void_p)
    have = {f for f, _ in TgnBuffers._fields_}
    assert set(fields) <= have and set(NODE_ROW_TENSORS) | {"store"} == set(fields)


def test_python_surface_exists_and_earlier_signatures_stand():
    import inspect

    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnEngine, TGNModel
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(TgnEngine.grow_nodes) == ["self", "n"] and par(TgnEngine.reserve_nodes) == ["self", "cap"]
    assert isinstance(TgnEngine.node_capacity, property) and isinstance(TGNModel.node_capacity, property)
    assert par(TGNModel.grow_nodes) == ["self", "n"]
    assert par(LastNeighborLoader.grow)[:2] == ["self", "num_nodes"]
    assert par(TgnEngine.append_events_grow) == ["self", "src", "dst", "t", "msg"]
    assert par(TgnEngine.load_stream_state_grow) == ["self", "state"]
    obs = inspect.signature(TgnEngine.observe_events).parameters
    assert list(obs)[-1] == "grow" and obs["grow"].default is False and obs["validate"].default is True
    assert par(tgn_epoch.grow_nodes) == ["model", "neighbor_loader", "n"]
    assert par(tgn_epoch.observe_grow) == par(tgn_epoch.observe)
    for name in ("grow_nodes", "observe_grow"):
        assert getattr(pyg_epoch_utils, name) is getattr(tgn_epoch, name)
    assert "dst_nodes" in TgnEngine.grow_nodes.__doc__ and "NOT extended" in TgnEngine.grow_nodes.__doc__
    # every new keyword defaults to the earlier path, and the entry points other tests pin keep their lists
    assert par(TgnEngine.append_events) == ["self", "src", "dst", "t", "msg", "validate"]
    assert par(TgnEngine.load_stream_state) == ["self", "state"]
    assert par(tgn_epoch.observe) == ["model", "neighbor_loader", "src", "dst", "t", "msg", "batch"]


def test_c_calls_check_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers, TgnGrowOut
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtgnx.so is not built here")
    L = _lib.lib()
    cfg = _tgn_cfg()
    keep = np.zeros(4096, dtype=np.float32)                # host memory: must never be touched
    p = ctypes.c_void_p(keep.ctypes.data)
    null = ctypes.c_void_p(0)
    rows = ("nbr", "eid", "rt", "assoc", "memory", "last_update", "node_gen", "store")

    def bufs(*zero):
        b = TgnBuffers()
        for f in rows:
            setattr(b, f, 0 if f in zero else p.value)
        return b

    def outs(*zero):
        o = TgnGrowOut()
        for f in rows:
            setattr(o, f, 0 if f in zero else p.value + 2048)
        return o

    def nodes(cfg_ref=None, b=None, n=301, cap=400, out=None, bad=p):
        return L.tgnx_tgn_grow_nodes(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                     ctypes.byref(bufs()) if b is None else b, n, cap,
                                     ctypes.byref(outs()) if out is None else out, bad, null)

    def store(cfg_ref=None, b=None, n=301, new=p, bad=p):
        return L.tgnx_tgn_grow_store(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                     ctypes.byref(bufs()) if b is None else b, n,
                                     ctypes.c_void_p(p.value + 2048) if new is p else new, bad, null)

    def failed(rc, code=-1):
        return rc == code and len(L.tgnx_last_error()) > 0

    for f in (nodes, store):
        assert failed(f(cfg_ref=null)) and failed(f(b=null)) and failed(f(bad=null))
        assert f.__name__.encode() in L.tgnx_last_error()
        assert failed(f(n=299)) and failed(f(n=0)) and failed(f(n=-1))            # nodes are never dropped
        assert failed(f(n=1 << 31), code=-3)
        assert failed(f(bad=ctypes.c_void_p(p.value + 4)))
        for bad in (dict(num_nodes=0), dict(ring=0), dict(num_events=0), dict(mem_dim=0)):
            assert failed(f(cfg_ref=ctypes.byref(_tgn_cfg(**bad)))), bad
    assert failed(nodes(out=null)) and failed(nodes(cap=300)) and failed(nodes(cap=1 << 31, n=301), code=-3)
    for field in rows:                                     # an old tensor without its new allocation, and the reverse
        assert failed(nodes(b=ctypes.byref(bufs(field)))), field
        assert failed(nodes(out=ctypes.byref(outs(field)))), field
    assert failed(nodes(b=ctypes.byref(bufs(*rows)), out=ctypes.byref(outs(*rows))))   # nothing to grow
    same = TgnGrowOut()
    for f in rows:
        setattr(same, f, p.value)
    assert failed(nodes(out=ctypes.byref(same)))           # growing in place is refused
    assert failed(store(new=null)) and failed(store(b=ctypes.byref(bufs("store")))) and failed(store(new=ctypes.c_void_p(p.value)))
    assert keep.sum() == 0


def test_grown_node_capacity():
    from tgnx.tgn import grown_node_capacity
    for cap in (0, 1, 2, 7, 64, 255, 256, 9227, 1 << 20):
        for need in range(0, cap + 1, max(cap // 7, 1)):
            assert grown_node_capacity(cap, need) == cap                   # unchanged while the need fits
        for need in (cap + 1, cap + 2, 2 * cap + 3, 10 * cap + 1):
            got = grown_node_capacity(cap, need)
            assert got >= need and got >= cap + cap // 4                   # >= need, and geometric
            assert grown_node_capacity(got, need) == got
    for cap in (1, 70, 300):                                               # monotone in the need
        vals = [grown_node_capacity(cap, need) for need in range(0, 4 * cap)]
        assert vals == sorted(vals)
    assert grown_node_capacity(70, 74) == 87 and grown_node_capacity(87, 93) == 108 and grown_node_capacity(87, 87) == 87
    # n nodes added one at a time copy O(n) rows in all: every reallocation copies the rows held then
    for n0, n in ((1, 20_000), (9227, 30_000)):
        cap, copied, reallocs = n0, 0, 0
        for need in range(n0 + 1, n0 + n + 1):
            new = grown_node_capacity(cap, need)
            if new != cap:
                copied, reallocs, cap = copied + need - 1, reallocs + 1, new
        assert cap >= n0 + n and copied <= 6 * (n0 + n) and reallocs <= 8 + 5 * int(np.log2((n0 + n) / n0 + 1))
    for bad in ((-1, 3), (3, -1)):
        with pytest.raises(ValueError):
            grown_node_capacity(*bad)


def test_argument_checks():
    from tgnx.tgn import check_append_args, check_grow_args
    assert check_grow_args(300, 300) is False and check_grow_args(300, 1) is False and check_grow_args(300, -5) is False
    assert check_grow_args(300, 301) is True and check_grow_args(1, (1 << 31) - 1) is True
    for kw in (dict(world=2), dict(dp=True), dict(world=8, dp=True)):
        for n in (10, 300, 301):                                           # refused whether or not it would grow
            with pytest.raises(ValueError, match="one device"):
                check_grow_args(300, n, **kw)
    for n in (1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="2\\^31"):
            check_grow_args(300, n)
    assert check_append_args(True, False) is None and check_append_args(False, False) is None
    assert check_append_args(True, True) is None
    with pytest.raises(ValueError, match="validate"):
        check_append_args(False, True)


def test_relaxed_stream_state_check_relaxes_num_nodes_only():
    from tgnx.tgn import check_stream_state, check_stream_state_grow
    fp = dict(num_nodes=3, ring=2, mem_dim=4, msg_dim=5)
    assert check_stream_state_grow(_state(), fp) == (6, 3)
    assert check_stream_state_grow(_state(N=7), fp) == (6, 7) and check_stream_state_grow(_state(N=1, n=0), fp) == (0, 1)
    for n in (7, 1):                                                       # the strict check still refuses both
        with pytest.raises(ValueError, match="fingerprint"):
            check_stream_state(_state(N=n), fp)
    for k, v in (("ring", 10), ("mem_dim", 8), ("msg_dim", 16)):
        with pytest.raises(ValueError, match="fingerprint"):
            check_stream_state_grow(_state(N=7), dict(fp, **{k: v}))
    with pytest.raises(ValueError, match="format"):
        check_stream_state_grow(_state(N=7, format=2), fp)
    with pytest.raises(ValueError, match="format"):
        check_stream_state_grow({"src": 1}, fp)
    with pytest.raises(ValueError):
        check_stream_state_grow([1, 2], fp)
    st = _state(N=7)
    del st["store_arena"]
    with pytest.raises(ValueError, match="missing"):
        check_stream_state_grow(st, fp)
    st = _state(N=7)
    del st["num_nodes"]
    with pytest.raises(ValueError, match="missing"):
        check_stream_state_grow(st, fp)
    for bad in (0, -2, 1 << 31):
        with pytest.raises(ValueError, match="num_nodes"):
            check_stream_state_grow(_state(num_nodes=bad), fp)
    # every shape is still checked, the [N, .] ones against the state's own num_nodes
    for k, v in (("msg", torch.zeros(6, 4)), ("src", torch.zeros(5, dtype=torch.long)),
                 ("store_arena", torch.zeros(6, dtype=torch.long)), ("e_id", torch.zeros(7, 3, dtype=torch.long)),
                 ("ctl", torch.zeros(8, dtype=torch.long)), ("memory", torch.zeros(3, 4)),
                 ("node_gen", torch.zeros(6, dtype=torch.int32)), ("store_nodes", torch.zeros(7, 2, dtype=torch.long))):
        with pytest.raises(ValueError, match=k):
            check_stream_state_grow(_state(N=7, **{k: v}), fp)
    with pytest.raises(ValueError, match="num_events"):
        check_stream_state_grow(_state(N=7, num_events=-1), fp)


def test_pad_reference_on_a_hand_made_state():
    g = torch.Generator().manual_seed(0)
    st = _state(N=3, K=2, D=4, d=5, n=6, memory=torch.rand(3, 4, generator=g),
                last_update=torch.tensor([5, 0, 9]), node_gen=torch.tensor([2, 0, 3], dtype=torch.int32),
                store_nodes=torch.tensor([[8, 2, 0, 0], [0, 0, 10, 2], [3, 1, 0, 0]]),
                store_arena=torch.tensor([0, 0, 1, 1, 2, 3, 2, 3, 4, 5, 4, 5]),
                neighbors=torch.tensor([[1, -1], [0, -1], [1, -1]]), e_id=torch.tensor([[5, -1], [5, -1], [1, -1]]),
                ring_t=torch.tensor([[3.0, -1.0], [3.0, -1.0], [1.0, -1.0]]), ctl=torch.arange(24))
    big = pad_state(st, 5)
    assert big["num_nodes"] == 5 and big["num_events"] == 6 and big["format"] == 1
    assert big["memory"].shape == (5, 4) and big["neighbors"].shape == (5, 2) and big["store_nodes"].shape == (5, 4)
    assert big["store_arena"].shape == (12,) and torch.equal(big["store_arena"], st["store_arena"])
    assert torch.equal(big["ctl"], st["ctl"])
    assert big["neighbors"][3:].tolist() == [[-1, -1]] * 2 and big["e_id"][3:].tolist() == [[-1, -1]] * 2
    assert big["ring_t"][3:].tolist() == [[-1.0, -1.0]] * 2 and big["ring_t"].dtype == torch.float32
    assert not big["memory"][3:].any() and not big["store_nodes"][3:].any() and big["node_gen"].dtype == torch.int32
    assert set(RESET_ROW) == {"memory", "last_update", "node_gen", "store_nodes", "neighbors", "e_id", "ring_t"}
    back, rest = crop_state(big, 3)
    assert same_state(back, st) == [] and same_state(st, back) == [] and is_reset_rows(rest)
    assert same_state(pad_state(st, 3), st) == []                              # growing by nothing
    assert same_state(pad_state(pad_state(st, 4), 5), big) == []               # two growths are one
    assert "memory" in same_state(big, pad_state(st, 6)) and "num_nodes" in same_state(big, st)
    touched = {k: v.clone() for k, v in rest.items()}
    touched["e_id"][0, 0] = 0
    assert not is_reset_rows(touched)
    other = dict(big, ctl=big["ctl"].clone())
    other["ctl"][3] += 1
    assert same_state(big, other) == ["ctl"] and same_state(big, other, skip_ctl=(3,)) == []
    with pytest.raises(ValueError):
        pad_state(st, 2)
    from tgnx.tgn import check_stream_state
    assert check_stream_state(big, dict(num_nodes=5, ring=2, mem_dim=4, msg_dim=5)) == 6
