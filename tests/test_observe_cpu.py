"""CPU checks of the score-free ingestion surface (tgnx_tgn_observe_step and what sits on it): the library exports
the entry point, its ctypes signature restates the header's argument list, the Python methods and the drop-in exist,
the argument check refuses null buffers before any device call (the pointers handed in are host memory, as in
test_query_cpu.py), and the host-side arithmetic of the growing event table — capacity growth, the shape check of an
appended chunk, the batch check of observe() — holds without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAME = "tgnx_tgn_observe_step"


def _header():
    return open(os.path.join(ROOT, "include", "tgnx.h")).read()


def test_library_exports_and_binds_the_entry_point():
    from tgnx import _lib
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.SIGNATURES
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % NAME, hdr)
    assert m and m.group(1) == "int"
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int
    decl = [a.strip() for a in m.group(2).split(",")]
    assert len(decl) == len(args) == 3 and all("*" in a for a in decl) and all(a is _lib.P for a in args)


def test_python_surface_exists():
    import inspect

    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.tgn import TgnEngine
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(TgnEngine.observe) == ["self", "start", "B"]
    assert par(TgnEngine.append_events) == ["self", "src", "dst", "t", "msg", "validate"]
    assert inspect.signature(TgnEngine.append_events).parameters["validate"].default is True
    assert par(TgnEngine.observe_events)[:6] == ["self", "src", "dst", "t", "msg", "batch"]
    assert inspect.signature(TgnEngine.observe_events).parameters["batch"].default is None
    assert par(TgnEngine.observe_range) == ["self", "lo", "hi", "batch"]
    assert par(TgnEngine.reserve_events) == ["self", "n"]
    assert isinstance(TgnEngine.num_events, property)
    assert par(tgn_epoch.observe) == ["model", "neighbor_loader", "src", "dst", "t", "msg", "batch"]
    assert pyg_epoch_utils.observe is tgn_epoch.observe


def _tgn_cfg(**kw):
    from tgnx.tgn import TgnConfig
    base = dict(num_nodes=300, num_events=600, ring=10, mem_dim=32, msg_dim=16, heads=2, max_batch=8, max_neg=1,
                aggr=0, dropout=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, layers=1, updater=0, emb_in_msg=0)
    base.update(kw)
    return TgnConfig(**base)


def test_observe_step_checks_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers
    L = _lib.lib()
    keep = np.zeros(256, dtype=np.float32)
    p = ctypes.c_void_p(keep.ctypes.data)
    null = ctypes.c_void_p(0)
    cfg = _tgn_cfg()

    def bufs(**zero):
        b = TgnBuffers()
        for f, _ in TgnBuffers._fields_:
            if f not in ("n_dst", "xcap", "flags", "xrows", "plan_table", "out_ev", "neg", "out_pos", "out_neg", "mrr"):
                setattr(b, f, 0 if f in zero else p.value)
        return b

    def failed(rc):
        return rc == -1 and len(L.tgnx_last_error()) > 0         # TGNX_EINVAL

    assert failed(L.tgnx_tgn_observe_step(null, ctypes.byref(bufs()), null))
    assert failed(L.tgnx_tgn_observe_step(ctypes.byref(cfg), null, null))
    assert b"tgnx_tgn_observe_step" in L.tgnx_last_error()
    for f in ("ctl", "ws", "memory", "last_update", "store", "node_gen", "nbr", "eid", "rt", "ev_src", "ev_dst", "ev_t",
              "ev_msg", "params"):
        assert failed(L.tgnx_tgn_observe_step(ctypes.byref(cfg), ctypes.byref(bufs(**{f: 1})), null)), f
    for bad in (dict(heads=3), dict(max_batch=0), dict(num_events=0), dict(layers=2, emb_in_msg=1), dict(ring=0)):
        assert failed(L.tgnx_tgn_observe_step(ctypes.byref(_tgn_cfg(**bad)), ctypes.byref(bufs()), null)), bad
    assert keep.sum() == 0


def test_grown_capacity():
    from tgnx.tgn import grown_capacity
    assert grown_capacity(300, 300) == 300 and grown_capacity(300, 0) == 300      # fits: unchanged
    assert grown_capacity(300, 301) == 450                                        # 1.5 x
    assert grown_capacity(300, 350) == 450 and grown_capacity(450, 451) == 675
    assert grown_capacity(300, 1000) == 1000                                      # a chunk beyond 1.5 x: what it needs
    assert grown_capacity(0, 1) == 1 and grown_capacity(1, 2) == 2 and grown_capacity(2, 3) == 3
    with pytest.raises(ValueError):
        grown_capacity(-1, 4)
    # geometric: appending one row at a time to a table of 2 rows reallocates O(log n) times and copies O(n) rows
    cap, rows, grows, copied = 2, 2, 0, 0
    for _ in range(100000):
        new = grown_capacity(cap, rows + 1)
        if new != cap:
            grows, copied, cap = grows + 1, copied + rows, new
        rows += 1
        assert cap >= rows
    assert grows <= 40 and copied <= 4 * rows      # log_1.5(50,000) = 27 growths; the copies sum to < 3 x the last one


def test_check_event_rows():
    from tgnx.tgn import check_event_rows
    assert check_event_rows(5, 5, 5, (5, 16), 16) == 5
    assert check_event_rows(0, 0, 0, (0, 16), 16) == 0
    assert check_event_rows(3, 3, 3, (3, 0), 0) == 3
    for bad in ((5, 4, 5, (5, 16)), (5, 5, 6, (5, 16)), (5, 5, 5, (5, 15)), (5, 5, 5, (4, 16)), (5, 5, 5, (80,)),
                (5, 5, 5, (5, 16, 1))):
        with pytest.raises(ValueError, match="append_events"):
            check_event_rows(*bad, 16)


def test_check_observe_args():
    from tgnx.tgn import check_observe_args
    check_observe_args(0, 50, 50, 600)
    check_observe_args(550, 50, 50, 600)
    check_observe_args(600, 0, 50, 600)
    check_observe_args(7, 1, 50, 600)
    for bad in ((0, 51, 50, 600), (551, 50, 50, 600), (-1, 5, 50, 600), (0, -1, 50, 600), (600, 1, 50, 600)):
        with pytest.raises(ValueError, match="observe"):
            check_observe_args(*bad)
    with pytest.raises(ValueError, match="world"):
        check_observe_args(0, 5, 50, 600, world=2)
