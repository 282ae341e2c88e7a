"""CPU checks of the read-only inference surface (tgnx_link_predictor_topk, tgnx_tgn_embed and what sits on them):
the library exports the entry points, their ctypes signatures restate the header's argument lists, the torch op is
listed and registered, the Python methods exist, and every bad argument is refused in the argument check — before
any device call (the pointers handed in are host memory, as in test_nn_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("tgnx_link_predictor_topk_ws_bytes", "tgnx_link_predictor_topk", "tgnx_tgn_embed_max_nodes", "tgnx_tgn_embed")
TOPK_MAX = 128


def _header():
    return open(os.path.join(ROOT, "include", "tgnx.h")).read()


def test_library_exports_the_query_entry_points():
    from tgnx import _lib
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert re.search(r"#define\s+TGNX_TOPK_MAX\s+%d\b" % TOPK_MAX, _header())


def _ctype_of(decl: str):
    from tgnx import _lib
    if "*" in decl:
        return _lib.P
    for name, ct in (("int64_t", _lib.c_i64), ("int32_t", _lib.c_i32), ("uint64_t", _lib.c_u64), ("size_t", _lib.c_sz)):
        if re.search(r"\b%s\b" % name, decl):
            return ct
    assert re.search(r"\bint\b", decl), decl
    return ctypes.c_int


@pytest.mark.parametrize("name", NEW)
def test_signatures_match_the_header(name):
    from tgnx import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, name
    res, args = _lib.SIGNATURES[name]
    assert res is _ctype_of(m.group(1)), (name, m.group(1))
    want = [_ctype_of(a) for a in m.group(2).split(",")]
    assert len(args) == len(want), (name, len(args), len(want))
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (name, i, a, w)


def test_torch_op_and_python_surface_exist():
    import inspect

    import pyg_epoch_utils
    from tgnx import ops, tgn_epoch
    from tgnx.nn import LinkPredictor
    from tgnx.tgn import TgnEngine
    ns = ops.load()
    assert "predictor_topk" in ops.OPS and hasattr(ns, "predictor_topk")
    assert "-> (Tensor, Tensor, Tensor)" in str(ns.predictor_topk.default._schema)
    sig = inspect.signature(ops.link_topk)
    assert list(sig.parameters)[:9] == ["z_src", "z_cand", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out", "k"]
    assert sig.parameters["sigmoid"].default is True and sig.parameters["return_scores"].default is False
    assert list(inspect.signature(LinkPredictor.topk).parameters) == ["self", "z_src", "z_cand", "k", "return_scores"]
    assert list(inspect.signature(TgnEngine.embed).parameters) == ["self", "nodes", "validate"]
    assert inspect.signature(TgnEngine.embed).parameters["validate"].default is True
    assert list(inspect.signature(TgnEngine.recommend).parameters) == ["self", "src", "k", "candidates", "return_scores"]
    assert list(inspect.signature(tgn_epoch.recommend).parameters) == ["model", "neighbor_loader", "src", "k", "candidates"]
    assert pyg_epoch_utils.recommend is tgn_epoch.recommend


def _buf(n=256):
    a = np.zeros(n, dtype=np.float32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _failed(L, rc, name):
    return rc != 0 and name in L.tgnx_last_error()


def test_link_predictor_topk_checks_arguments_before_any_device_call():
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    name = b"tgnx_link_predictor_topk"
    need = L.tgnx_link_predictor_topk_ws_bytes(3, 5, 4, 4, 2)
    assert need > 0

    def call(n_src=3, n_cand=5, d_in=4, D=4, z_src=p, z_cand=p, w_src=p, b_src=p, w_dst=p, b_dst=p, w_out=p, b_out=p,
             k=2, out_val=p, out_idx=p, out_all=null, ws=p, ws_bytes=None):
        nb = L.tgnx_link_predictor_topk_ws_bytes(n_src, n_cand, d_in, D, k) if ws_bytes is None else ws_bytes
        return L.tgnx_link_predictor_topk(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w_out,
                                          b_out, k, 1, out_val, out_idx, out_all, ws, nb, null)

    for bad in (dict(k=0), dict(k=TOPK_MAX + 1), dict(n_src=-1), dict(n_cand=-1), dict(D=257), dict(d_in=0),
                dict(z_src=null), dict(z_cand=null), dict(w_src=null), dict(w_dst=null), dict(w_out=null),
                dict(b_out=null), dict(out_val=null), dict(out_idx=null), dict(ws=null), dict(ws_bytes=need - 1)):
        assert _failed(L, call(**bad), name), bad
    assert b"workspace" in L.tgnx_last_error()
    assert b"k must be" in (call(k=0), L.tgnx_last_error())[1]
    assert keep.sum() == 0


def test_link_predictor_topk_ws_bytes_is_monotone_in_n_cand():
    from tgnx import _lib
    L = _lib.lib()
    for n_src, D, k in ((1, 100, 10), (200, 100, 10), (5, 32, 128), (4000, 100, 64)):
        sizes = [L.tgnx_link_predictor_topk_ws_bytes(n_src, n, D, D, k)
                 for n in list(range(0, 1300)) + list(range(1300, 400000, 997))]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n_src, D, k)
        assert sizes[-1] > sizes[0]
    # Hs, Hd and the partial (value, position) lists at least
    assert L.tgnx_link_predictor_topk_ws_bytes(200, 9227, 100, 100, 10) >= (200 + 9227) * 100 * 4 + 200 * 19 * 10 * 8


def _tgn_cfg(**kw):
    from tgnx.tgn import TgnConfig
    base = dict(num_nodes=300, num_events=600, ring=10, mem_dim=32, msg_dim=16, heads=2, max_batch=8, max_neg=1,
                aggr=0, dropout=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, layers=1, updater=0, emb_in_msg=0)
    base.update(kw)
    return TgnConfig(**base)


def test_tgn_embed_checks_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    name = b"tgnx_tgn_embed"
    cfg = _tgn_cfg()
    assert L.tgnx_tgn_embed_max_nodes(ctypes.byref(cfg)) == 24          # min(N, max_batch * (2 + max_neg))
    assert L.tgnx_tgn_embed_max_nodes(ctypes.byref(_tgn_cfg(max_batch=200, max_neg=5))) == 300    # capped at N
    assert L.tgnx_tgn_embed_max_nodes(ctypes.byref(_tgn_cfg(max_neg=0))) == 24
    assert L.tgnx_tgn_embed_max_nodes(null) == 0
    b = TgnBuffers()
    for f, _ in TgnBuffers._fields_:
        if f not in ("n_dst", "xcap", "flags", "xrows", "plan_table", "out_ev"):
            setattr(b, f, p.value)
    cr, br = ctypes.byref(cfg), ctypes.byref(b)
    assert _failed(L, L.tgnx_tgn_embed(null, br, p, 4, p, null, null), name)
    assert _failed(L, L.tgnx_tgn_embed(cr, null, p, 4, p, null, null), name)
    assert _failed(L, L.tgnx_tgn_embed(cr, br, p, 25, p, null, null), name)      # n = capacity + 1
    assert b"tgnx_tgn_embed_max_nodes" in L.tgnx_last_error()
    assert _failed(L, L.tgnx_tgn_embed(cr, br, p, -1, p, null, null), name)
    assert _failed(L, L.tgnx_tgn_embed(cr, br, null, 4, p, null, null), name)
    assert _failed(L, L.tgnx_tgn_embed(cr, br, p, 4, null, null, null), name)
    assert L.tgnx_tgn_embed(cr, br, p, 0, p, null, null) == 0                      # nothing to do: no launch
    assert keep.sum() == 0
