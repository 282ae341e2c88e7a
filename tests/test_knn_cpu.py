"""CPU checks of the embedding-space nearest-neighbour surface (tgnx_embed_knn, torch.ops.tgnx.embed_knn,
tgnx.ops.embed_knn, TgnEngine.similar, pyg_epoch_utils.similar): the numpy reference the GPU tests compare with
(tests/knn_ref.py) on hand cases — ties to the lower position, a NaN row never selected, a zero row scoring 0 under
cosine, k > n_cand padding, exclude-self through duplicated candidates — and, without a device, the signatures, the
metric-name and k checks, the C ABI declared / exported / bound with matching ctypes, every bad argument refused
before any device call (the pointers handed in are host memory), a workspace size monotone in n_cand, and the op
registered with the documented schema."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("tgnx_embed_knn_ws_bytes", "tgnx_embed_knn")
TOPK_MAX = 128


# ---------------------------------------------------------------- the reference, by hand
def test_ties_go_to_the_lower_position():
    from knn_ref import knn
    zq = np.array([[1.0, 0.0]])
    zc = np.array([[0.5, 3.0], [1.0, 1.0], [1.0, -2.0], [0.5, 0.0], [1.0, 7.0]])    # dot: .5 1 1 .5 1
    idx, val, s = knn(zq, zc, 4, "dot")
    assert s.tolist() == [[0.5, 1.0, 1.0, 0.5, 1.0]]
    assert idx.tolist() == [[1, 2, 4, 0]] and val.tolist() == [[1.0, 1.0, 1.0, 0.5]]
    # -0 equals +0: position decides
    idx, _, _ = knn(np.array([[1.0, 0.0]]), np.array([[0.0, 1.0], [-0.0, 1.0]]), 2, "dot")
    assert idx.tolist() == [[0, 1]]


def test_a_nan_row_is_never_selected():
    from knn_ref import knn
    zq = np.array([[1.0, 2.0]])
    zc = np.array([[1.0, 0.0], [np.nan, 1.0], [-1.0, -1.0]])
    for metric in ("dot", "cosine"):
        idx, val, s = knn(zq, zc, 3, metric)
        assert np.isnan(s[0, 1]) and not np.isnan(s[0, [0, 2]]).any()
        assert idx.tolist() == [[0, 2, -1]] and np.isneginf(val[0, 2])
    # a NaN query: nothing is selected
    idx, val, _ = knn(np.array([[np.nan, 1.0]]), zc, 2, "cosine")
    assert idx.tolist() == [[-1, -1]] and np.isneginf(val).all()


def test_a_zero_row_scores_zero_under_cosine():
    from knn_ref import knn, scores
    zq = np.array([[3.0, 4.0], [0.0, 0.0]])
    zc = np.array([[0.0, 0.0], [6.0, 8.0], [-3.0, -4.0], [0.0, -5.0]])
    s = scores(zq, zc, "cosine")
    assert not np.isnan(s).any()
    assert np.allclose(s[0], [0.0, 1.0, -1.0, -0.8]) and (s[1] == 0).all() and (s[:, 0] == 0).all()
    idx, val, _ = knn(zq, zc, 2, "cosine")
    assert idx[0].tolist() == [1, 0] and idx[1].tolist() == [0, 1]         # the zero query: all ties, positions
    assert np.allclose(val[0], [1.0, 0.0])
    assert scores(zq, zc, "dot")[0].tolist() == [0.0, 50.0, -25.0, -20.0]
    with pytest.raises(ValueError):
        scores(zq, zc, "euclid")


def test_k_beyond_the_candidates_pads():
    from knn_ref import knn
    rng = np.random.default_rng(0)
    zq, zc = rng.standard_normal((3, 5)), rng.standard_normal((2, 5))
    idx, val, s = knn(zq, zc, 4, "cosine")
    assert (idx[:, 2:] == -1).all() and np.isneginf(val[:, 2:]).all()
    assert all(sorted(idx[q, :2].tolist()) == [0, 1] for q in range(3))
    assert (val[:, 0] >= val[:, 1]).all() and (np.abs(s) <= 1 + 1e-12).all()
    idx, val, s = knn(zq, np.zeros((0, 5)), 2, "dot")
    assert s.shape == (3, 0) and (idx == -1).all() and np.isneginf(val).all()


def test_exclude_self_applies_through_duplicated_candidates():
    from knn_ref import knn
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((6, 4))
    cand = np.array([3, 0, 3, 5, 1, 0, 3])                     # node 3 three times, node 0 twice
    nodes = np.array([3, 0, 2])
    idx, val, s = knn(emb[nodes], emb[cand], 7, "cosine", cand_key=cand, q_key=nodes)
    assert np.allclose(s[0, [0, 2, 6]], 1.0) and np.allclose(s[1, [1, 5]], 1.0)
    assert set(idx[0].tolist()) == {1, 3, 4, 5, -1} and (idx[0, 4:] == -1).all()        # every copy of node 3 gone
    assert set(idx[1].tolist()) == {0, 2, 3, 4, 6, -1} and (idx[1, 5:] == -1).all()
    assert (idx[2] >= 0).all()                                                          # node 2 is no candidate
    # an exclusion segment on top: query 0 also loses node 0, query 2 loses all but one node
    ptr, keys = np.array([0, 1, 1, 4]), np.array([0, 0, 1, 3])
    idx, _, _ = knn(emb[nodes], emb[cand], 3, "dot", cand_key=cand, q_key=nodes, excl_ptr=ptr, excl_key=keys)
    assert set(idx[0].tolist()) == {3, 4, -1} and idx[2].tolist() == [3, -1, -1]


# ---------------------------------------------------------------- the surface, without a device
def _header():
    return open(os.path.join(ROOT, "include", "tgnx.h")).read()


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
def test_entry_points_are_declared_exported_and_bound(name):
    from tgnx import _lib
    L = _lib.lib()
    assert hasattr(L, name) and name in _lib.SIGNATURES
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, name
    res, args = _lib.SIGNATURES[name]
    assert res is _ctype_of(m.group(1))
    want = [_ctype_of(a) for a in m.group(2).split(",")]
    assert len(args) == len(want), (name, len(args), len(want))
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (name, i, a, w)


def test_metric_codes_and_k_range_match_the_header():
    from tgnx import ops
    hdr = _header()
    for name, code in (("dot", "TGNX_KNN_DOT"), ("cosine", "TGNX_KNN_COSINE")):
        assert int(re.search(r"#define %s (\d+)" % code, hdr).group(1)) == ops.KNN_METRICS[name]
    assert int(re.search(r"#define TGNX_TOPK_MAX (\d+)", hdr).group(1)) == ops.TOPK_MAX == TOPK_MAX
    assert ops.knn_metric("cosine") == 1 and ops.knn_metric("dot") == 0
    for bad in ("euclidean", "Cosine", None, 1):
        with pytest.raises(ValueError):
            ops.knn_metric(bad)
    assert ops.knn_k(1) == 1 and ops.knn_k(TOPK_MAX) == TOPK_MAX
    for bad in (0, -3, TOPK_MAX + 1):
        with pytest.raises(ValueError):
            ops.knn_k(bad)


def test_embed_knn_refuses_an_unknown_metric_and_k_before_touching_the_operands():
    import torch

    from tgnx import ops
    z = torch.zeros(2, 4)                      # CPU tensors: the op itself would refuse them
    with pytest.raises(ValueError):
        ops.embed_knn(z, z, 1, metric="manhattan")
    with pytest.raises(ValueError):
        ops.embed_knn(z, z, 0)
    with pytest.raises(ValueError):
        ops.embed_knn(z, z, TOPK_MAX + 1, metric="dot")


def test_torch_op_and_python_signatures():
    import pyg_epoch_utils
    from tgnx import ops, tgn_epoch
    from tgnx.tgn import TgnEngine
    ns = ops.load()
    assert "embed_knn" in ops.OPS and hasattr(ns, "embed_knn")
    s = str(ns.embed_knn.default._schema)
    assert "embed_knn(Tensor z_q, Tensor z_cand, int metric, int k, bool return_scores, Tensor? cand_key, " \
           "Tensor? q_key, Tensor? excl_ptr, Tensor? excl_key) -> (Tensor, Tensor, Tensor)" in s
    p = inspect.signature(ops.embed_knn).parameters
    assert list(p) == ["z_q", "z_cand", "k", "metric", "return_scores", "cand_key", "q_key", "exclude", "validate"]
    for kw, default in (("metric", "cosine"), ("return_scores", False), ("cand_key", None), ("q_key", None),
                        ("exclude", None), ("validate", True)):
        assert p[kw].default == default, kw
    p = inspect.signature(TgnEngine.similar).parameters
    assert list(p) == ["self", "nodes", "k", "candidates", "metric", "exclude_self", "exclude_seen", "exclude", "cached",
                       "return_scores"]
    assert p["candidates"].default is None
    for kw, default in (("metric", "cosine"), ("exclude_self", True), ("exclude_seen", False), ("exclude", None),
                        ("cached", False), ("return_scores", False)):
        assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY and p[kw].default == default, kw
    p = inspect.signature(tgn_epoch.similar).parameters
    assert list(p) == ["model", "neighbor_loader", "nodes", "k", "candidates", "metric", "exclude_self", "exclude_seen",
                       "exclude", "cached"]
    for kw, default in (("metric", "cosine"), ("exclude_self", True), ("exclude_seen", False), ("exclude", None),
                        ("cached", False)):
        assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY and p[kw].default == default, kw
    assert pyg_epoch_utils.similar is tgn_epoch.similar


def _buf(n=256):
    a = np.zeros(n, dtype=np.float32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_embed_knn_checks_arguments_before_any_device_call():
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    need = L.tgnx_embed_knn_ws_bytes(3, 5, 4, 2)
    assert need >= (3 + 5) * 4 * 4 + 3 * 1 * 2 * 8

    def call(n_q=3, n_cand=5, D=4, z_q=p, z_cand=p, metric=1, k=2, cand_key=null, q_key=null, excl_ptr=null,
             excl_key=null, nnz=0, out_val=p, out_idx=p, out_all=null, ws=p, ws_bytes=None):
        nb = L.tgnx_embed_knn_ws_bytes(n_q, n_cand, D, k) if ws_bytes is None else ws_bytes
        return L.tgnx_embed_knn(n_q, n_cand, D, z_q, z_cand, metric, k, cand_key, q_key, excl_ptr, excl_key, nnz,
                                out_val, out_idx, out_all, ws, nb, null)

    for bad in (dict(k=0), dict(k=TOPK_MAX + 1), dict(n_q=-1), dict(n_cand=-1), dict(D=0), dict(D=257),
                dict(metric=2), dict(metric=-1), dict(nnz=-1), dict(excl_ptr=p, nnz=3), dict(z_q=null),
                dict(z_cand=null), dict(out_val=null), dict(out_idx=null), dict(ws=null),
                dict(ws=ctypes.c_void_p(keep.ctypes.data + 4)), dict(ws_bytes=need - 1)):
        rc = call(**bad)
        assert rc == -1 and b"tgnx_embed_knn" in L.tgnx_last_error(), bad          # TGNX_EINVAL
    assert b"workspace" in L.tgnx_last_error()
    assert call(n_q=0) == 0                                   # nothing to do: no launch
    assert keep.sum() == 0


def test_ws_bytes_is_monotone_in_n_cand():
    from tgnx import _lib
    L = _lib.lib()
    for n_q, D, k in ((1, 100, 10), (200, 100, 10), (5, 256, 128), (17, 3, 1)):
        ns = list(range(0, 1300)) + list(range(1300, 400000, 997))
        sizes = [L.tgnx_embed_knn_ws_bytes(n_q, n, D, k) for n in ns]
        assert all(y >= x for x, y in zip(sizes, sizes[1:])), (n_q, D, k)
        assert sizes[-1] > sizes[0]
    # both operands at the padded pitch and the partial lists of every 256-candidate chunk
    assert L.tgnx_embed_knn_ws_bytes(200, 9227, 100, 10) >= (200 + 9227) * 100 * 4 + 200 * 37 * 10 * 8
    assert L.tgnx_embed_knn_ws_bytes(200, 9227, 30, 10) >= (200 + 9227) * 32 * 4
    for bad in ((-1, 5, 4, 2), (3, -1, 4, 2), (3, 5, 0, 2), (3, 5, 257, 2), (3, 5, 4, 0), (3, 5, 4, TOPK_MAX + 1)):
        assert L.tgnx_embed_knn_ws_bytes(*bad) == 256
