"""CPU checks of the filtered and per-source-list top-k surface (tgnx_link_predictor_topk_filtered,
tgnx_link_predictor_topk_lists and what sits on them): the library exports the entry points and the header declares
them with the ctypes signatures, the two torch ops are registered with the documented schemas, every bad argument is
refused in the argument check — before any device call (the pointers handed in are host memory) — the workspace
sizes are monotone, and the numpy reference the GPU tests compare with (tests/topk_filter_ref.py) agrees with a
brute-force set-based restatement on random small inputs with ties, empty segments and keys matching nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("tgnx_link_predictor_topk_filtered_ws_bytes", "tgnx_link_predictor_topk_filtered",
       "tgnx_link_predictor_topk_lists_ws_bytes", "tgnx_link_predictor_topk_lists")
TOPK_MAX = 128


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
def test_entry_points_are_exported_and_declared(name):
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


def test_torch_ops_and_python_surface():
    import inspect

    import pyg_epoch_utils
    from tgnx import ops, tgn_epoch
    from tgnx.nn import LinkPredictor
    from tgnx.tgn import TgnEngine
    ns = ops.load()
    for name in ("predictor_topk_filtered", "predictor_topk_lists"):
        assert name in ops.OPS and hasattr(ns, name), name
    s = str(ns.predictor_topk_filtered.default._schema)
    assert "Tensor? cand_key, Tensor? src_key, Tensor? excl_ptr, Tensor? excl_key) -> (Tensor, Tensor, Tensor)" in s
    s = str(ns.predictor_topk_lists.default._schema)
    assert "Tensor list_ptr, Tensor list_idx, int max_len) -> (Tensor, Tensor, Tensor, Tensor, Tensor)" in s
    p = inspect.signature(ops.link_topk).parameters
    for kw, default in (("cand_key", None), ("src_key", None), ("exclude", None), ("lists", None), ("validate", True)):
        assert p[kw].default is default, kw
    for fn in (LinkPredictor.topk_filtered, TgnEngine.recommend_filtered, tgn_epoch.recommend_filtered):
        q = inspect.signature(fn).parameters
        for kw in ("cand_key", "src_key", "exclude", "lists") if fn is LinkPredictor.topk_filtered else \
                ("exclude_seen", "exclude_self", "exclude", "per_source"):
            assert q[kw].kind is inspect.Parameter.KEYWORD_ONLY, (fn, kw)
    assert list(inspect.signature(TgnEngine.score).parameters) == ["self", "src", "dst"]
    assert pyg_epoch_utils.recommend_filtered is tgn_epoch.recommend_filtered


def _buf(n=256):
    a = np.zeros(n, dtype=np.float32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _failed(L, rc, name):
    return rc == -1 and name in L.tgnx_last_error()          # TGNX_EINVAL


def test_filtered_checks_arguments_before_any_device_call():
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    name = b"tgnx_link_predictor_topk_filtered"
    need = L.tgnx_link_predictor_topk_filtered_ws_bytes(3, 5, 4, 4, 2)
    assert need == L.tgnx_link_predictor_topk_ws_bytes(3, 5, 4, 4, 2)

    def call(n_src=3, n_cand=5, d_in=4, D=4, z_src=p, z_cand=p, w_src=p, b_src=p, w_dst=p, b_dst=p, w_out=p, b_out=p,
             k=2, cand_key=null, src_key=null, excl_ptr=null, excl_key=null, nnz=0, out_val=p, out_idx=p, out_all=null,
             ws=p, ws_bytes=None):
        nb = L.tgnx_link_predictor_topk_filtered_ws_bytes(n_src, n_cand, d_in, D, k) if ws_bytes is None else ws_bytes
        return L.tgnx_link_predictor_topk_filtered(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst,
                                                   w_out, b_out, k, 1, cand_key, src_key, excl_ptr, excl_key, nnz,
                                                   out_val, out_idx, out_all, ws, nb, null)

    for bad in (dict(k=0), dict(k=TOPK_MAX + 1), dict(n_src=-1), dict(n_cand=-1), dict(D=257), dict(d_in=0),
                dict(nnz=-1), dict(excl_ptr=p, nnz=3), dict(z_src=null), dict(z_cand=null), dict(w_src=null),
                dict(w_dst=null), dict(w_out=null), dict(b_out=null), dict(out_val=null), dict(out_idx=null),
                dict(ws=null), dict(ws_bytes=need - 1)):
        assert _failed(L, call(**bad), name), bad
    assert b"workspace" in L.tgnx_last_error()
    assert call(n_src=0) == 0                                 # nothing to do: no launch
    assert keep.sum() == 0


def test_lists_checks_arguments_before_any_device_call():
    from tgnx import _lib
    L = _lib.lib()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    name = b"tgnx_link_predictor_topk_lists"
    need = L.tgnx_link_predictor_topk_lists_ws_bytes(3, 5, 4, 4, 2, 7)
    assert need > 0

    def call(n_src=3, n_cand=5, d_in=4, D=4, z_src=p, z_cand=p, w_src=p, b_src=p, w_dst=p, b_dst=p, w_out=p, b_out=p,
             k=2, list_ptr=p, list_idx=p, nnz=9, max_len=7, out_val=p, out_idx=p, out_slot=p, out_logits=null,
             n_invalid=null, ws=p, ws_bytes=None):
        nb = L.tgnx_link_predictor_topk_lists_ws_bytes(n_src, n_cand, d_in, D, k, max_len) if ws_bytes is None \
            else ws_bytes
        return L.tgnx_link_predictor_topk_lists(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst,
                                                w_out, b_out, k, 1, list_ptr, list_idx, nnz, max_len, out_val, out_idx,
                                                out_slot, out_logits, n_invalid, ws, nb, null)

    for bad in (dict(k=0), dict(k=TOPK_MAX + 1), dict(n_src=-1), dict(n_cand=-1), dict(D=257), dict(d_in=0),
                dict(nnz=-1), dict(max_len=-1), dict(list_ptr=null), dict(list_idx=null), dict(z_src=null),
                dict(z_cand=null), dict(w_src=null), dict(w_dst=null), dict(w_out=null), dict(b_out=null),
                dict(out_val=null), dict(out_idx=null), dict(out_slot=null), dict(ws=null), dict(ws_bytes=need - 1)):
        assert _failed(L, call(**bad), name), bad
    assert b"workspace" in L.tgnx_last_error()
    assert call(n_src=0) == 0
    assert keep.sum() == 0


def test_ws_bytes_are_monotone():
    from tgnx import _lib
    L = _lib.lib()
    for n_src, D, k in ((1, 100, 10), (200, 100, 10), (5, 32, 128)):
        ns = list(range(0, 1300)) + list(range(1300, 400000, 997))
        f = [L.tgnx_link_predictor_topk_filtered_ws_bytes(n_src, n, D, D, k) for n in ns]
        a = [L.tgnx_link_predictor_topk_lists_ws_bytes(n_src, n, D, D, k, 500) for n in ns]
        b = [L.tgnx_link_predictor_topk_lists_ws_bytes(n_src, 9227, D, D, k, n) for n in ns]
        for sizes in (f, a, b):
            assert all(y >= x for x, y in zip(sizes, sizes[1:])), (n_src, D, k)
            assert sizes[-1] > sizes[0]
    # Hs, Hd and two chunks of partial (value, slot) lists at least
    assert L.tgnx_link_predictor_topk_lists_ws_bytes(200, 9227, 100, 100, 10, 500) >= \
        (200 + 9227) * 100 * 4 + 200 * 2 * 10 * 8


def _brute_filtered(logits, cand_key, src_key, excl_ptr, excl_key, k):
    """Set-based restatement: drop, then repeatedly take the largest remaining entry (first position on a tie)."""
    n_src, n_cand = logits.shape
    idx, val = np.full((n_src, k), -1, np.int64), np.full((n_src, k), -np.inf, np.float32)
    for q in range(n_src):
        banned = set()
        if excl_ptr is not None:
            banned = set(int(x) for x in excl_key[excl_ptr[q]:excl_ptr[q + 1]])
        if src_key is not None:
            banned.add(int(src_key[q]))
        left = [c for c in range(n_cand) if int(c if cand_key is None else cand_key[c]) not in banned
                and not np.isnan(logits[q, c])]
        for r in range(min(k, len(left))):
            best = left[0]
            for c in left:
                if logits[q, c] > logits[q, best]:
                    best = c
            left.remove(best)
            idx[q, r], val[q, r] = best, logits[q, best]
    return idx, val


def test_reference_agrees_with_a_brute_force_restatement():
    from topk_filter_ref import filtered_topk, lists_topk
    rng = np.random.default_rng(0)
    for trial in range(60):
        n_src, n_cand, k = int(rng.integers(1, 6)), int(rng.integers(1, 14)), int(rng.integers(1, 9))
        logits = rng.integers(-3, 4, (n_src, n_cand)).astype(np.float32)          # few values: many ties
        if trial % 5 == 0:
            logits[rng.random(logits.shape) < 0.2] = np.nan
        cand_key = None if trial % 3 == 0 else rng.integers(0, n_cand, n_cand)   # duplicated keys
        src_key = None if trial % 4 == 0 else rng.integers(0, n_cand + 3, n_src)
        lens = rng.integers(0, 5, n_src) * (rng.random(n_src) < 0.7)              # empty segments
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = np.concatenate([np.sort(rng.integers(-2, n_cand + 4, n)) for n in lens] + [np.zeros(0, np.int64)])
        if trial % 7 == 0:
            ptr = None
        got = filtered_topk(logits, cand_key, src_key, ptr, keys, k)
        want = _brute_filtered(logits, cand_key, src_key, ptr, keys, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), trial
        # the ragged form: every row its own segment, masked entries NaN
        masked = logits.copy()
        masked[np.isnan(masked)] = np.nan
        flat_ptr = np.arange(n_src + 1) * n_cand
        slot, val = lists_topk(masked.reshape(-1), flat_ptr, k)
        want = _brute_filtered(masked, None, None, None, None, k)
        assert np.array_equal(slot, want[0]) and np.array_equal(val, want[1]), trial
    slot, val = lists_topk(np.zeros(0, np.float32), np.zeros(3, np.int64), 2)      # empty lists: padding
    assert (slot == -1).all() and np.isneginf(val).all()


def test_seen_lists_ignores_slots_without_an_event():
    from topk_filter_ref import seen_lists
    neighbors = np.array([[5, 9, 7, 3], [4, 4, 8, 1], [2, 6, 0, 0]], dtype=np.int64)
    e_id = np.array([[10, -1, 12, -1], [-1, -1, -1, -1], [3, 4, 5, 6]], dtype=np.int64)   # 9, 3 and row 1: stale ids
    ptr, keys = seen_lists(neighbors, e_id, [0, 1, 2, 0])
    assert ptr.tolist() == [0, 2, 2, 6, 8]
    assert keys.tolist() == [5, 7, 0, 0, 2, 6, 5, 7]


def test_link_topk_validates_ragged_arguments_on_the_host_side():
    """ops._ragged: the checks `validate` makes (CPU tensors: no device needed)."""
    import torch

    from tgnx import ops
    cpu = torch.device("cpu")
    ok = ops._ragged(([0, 2, 2, 5], [1, 4, 0, 3, 3]), 3, cpu, "exclude", True, True)
    assert ok[2] == 3
    for ptr, vals, srt in (([1, 2, 2, 5], [1, 4, 0, 3, 3], True), ([0, 3, 2, 5], [1, 4, 0, 3, 3], False),
                           ([0, 2, 2, 4], [1, 4, 0, 3, 3], False), ([0, 2, 2, 5], [4, 1, 0, 3, 3], True)):
        with pytest.raises(ValueError):
            ops._ragged((ptr, vals), 3, cpu, "exclude", True, srt)
    assert ops._ragged(([0, 2, 2, 5], [4, 1, 0, 3, 3]), 3, cpu, "lists", True, False)[2] == 3     # lists: any order
    with pytest.raises(ValueError):
        ops._ragged(([0, 5], [1, 2, 3, 4, 5]), 3, cpu, "lists", False, False)                    # n_src + 1 entries
