"""CPU checks of the link-rank surface (tgnx_link_predictor_rank and what sits on it): the library exports the entry
points and the header declares them with the ctypes signatures, the torch op is registered with the documented
schema, every bad argument is refused in the argument check — before any device call (the pointers handed in are
host memory) — the workspace size is monotone in n_cand, and the numpy reference the GPU tests compare with
(tests/link_rank_ref.py) gives TGB's ranks (oracle/mrr_ref.py) in the one-target-against-negatives setting and
follows the tie, NaN and duplicate-key rules on hand-made rows."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("tgnx_link_predictor_rank_ws_bytes", "tgnx_link_predictor_rank")


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
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tgnx.h")).read(), flags=re.S)
    m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, name
    res, args = _lib.SIGNATURES[name]
    assert res is _ctype_of(m.group(1))
    want = [_ctype_of(a) for a in m.group(2).split(",")]
    assert len(args) == len(want), (name, len(args), len(want))
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (name, i, a, w)


def test_torch_op_and_python_surface():
    import pyg_epoch_utils
    from tgnx import ops, tgn_epoch
    from tgnx.nn import LinkPredictor
    from tgnx.tgn import TgnEngine
    ns = ops.load()
    assert "predictor_rank" in ops.OPS and hasattr(ns, "predictor_rank")
    s = str(ns.predictor_rank.default._schema)
    assert "Tensor target, int n_count, Tensor? cand_key, Tensor? src_key, Tensor? excl_ptr, Tensor? excl_key) -> " \
           "(Tensor, Tensor, Tensor, Tensor)" in s
    p = inspect.signature(ops.link_rank).parameters
    assert list(p)[:9] == ["z_src", "z_cand", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out", "target"]
    for kw, default in (("n_count", None), ("cand_key", None), ("src_key", None), ("exclude", None), ("validate", True)):
        assert p[kw].default is default, kw
    assert list(inspect.signature(LinkPredictor.rank).parameters)[:4] == ["self", "z_src", "z_cand", "target"]
    p = inspect.signature(TgnEngine.rank).parameters
    assert list(p)[:5] == ["self", "src", "dst", "candidates", "return_scores"]
    q = inspect.signature(TgnEngine.rank_events).parameters
    assert list(q)[:4] == ["self", "start", "B", "candidates"]
    r = inspect.signature(tgn_epoch.rank_stream).parameters
    assert list(r)[:7] == ["model", "neighbor_loader", "lo", "hi", "batch", "candidates", "ks"]
    assert r["ks"].default == (1, 10, 50)
    for sig, kws in ((p, ("exclude_seen", "exclude_self", "exclude")), (q, ("exclude_seen", "exclude_self", "exclude")),
                     (r, ("exclude_seen", "exclude_self"))):
        for kw in kws:
            assert sig[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw
    assert pyg_epoch_utils.rank_stream is tgn_epoch.rank_stream


def _failed(L, rc, name):
    return rc == -1 and name in L.tgnx_last_error()          # TGNX_EINVAL


def test_rank_checks_arguments_before_any_device_call():
    from tgnx import _lib
    L = _lib.lib()
    keep = np.zeros(256, dtype=np.float32)
    p, null = ctypes.c_void_p(keep.ctypes.data), ctypes.c_void_p(0)
    name = b"tgnx_link_predictor_rank"
    need = L.tgnx_link_predictor_rank_ws_bytes(3, 5, 4, 4)
    assert need > 0

    def call(n_src=3, n_cand=5, d_in=4, D=4, z_src=p, z_cand=p, w_src=p, b_src=p, w_dst=p, b_dst=p, w_out=p, b_out=p,
             n_count=5, target=p, cand_key=null, src_key=null, excl_ptr=null, excl_key=null, nnz=0, out_gt=p, out_eq=p,
             out_n=p, out_tlogit=p, ws=p, ws_bytes=None):
        nb = L.tgnx_link_predictor_rank_ws_bytes(n_src, n_cand, d_in, D) if ws_bytes is None else ws_bytes
        return L.tgnx_link_predictor_rank(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w_out,
                                          b_out, n_count, target, cand_key, src_key, excl_ptr, excl_key, nnz, out_gt,
                                          out_eq, out_n, out_tlogit, ws, nb, null)

    for bad in (dict(n_src=-1), dict(n_cand=-1, n_count=0), dict(D=257), dict(d_in=0), dict(n_count=6),
                dict(n_count=-1), dict(nnz=-1), dict(excl_ptr=p, nnz=3), dict(z_src=null), dict(z_cand=null),
                dict(w_src=null), dict(w_dst=null), dict(w_out=null), dict(b_out=null), dict(target=null),
                dict(out_gt=null), dict(out_eq=null), dict(out_n=null), dict(out_tlogit=null), dict(ws=null),
                dict(ws_bytes=need - 1)):
        assert _failed(L, call(**bad), name), bad
    assert b"workspace" in L.tgnx_last_error()
    assert _failed(L, call(n_count=6), name) and b"n_count" in L.tgnx_last_error()
    assert call(n_src=0) == 0                                 # nothing to do: no launch
    assert keep.sum() == 0


def test_ws_bytes_is_monotone_in_n_cand():
    from tgnx import _lib
    L = _lib.lib()
    for n_src, D in ((1, 100), (200, 100), (5, 32)):
        ns = list(range(0, 1300)) + list(range(1300, 400000, 997))
        sizes = [L.tgnx_link_predictor_rank_ws_bytes(n_src, n, D, D) for n in ns]
        assert all(y >= x for x, y in zip(sizes, sizes[1:])), (n_src, D)
        assert sizes[-1] > sizes[0]
    assert L.tgnx_link_predictor_rank_ws_bytes(200, 9227, 100, 100) >= (200 + 9227) * 100 * 4    # Hs and Hd at least
    # no per-chunk partial lists: smaller than the top-k operator's at k = 1
    assert L.tgnx_link_predictor_rank_ws_bytes(200, 9227, 100, 100) < \
        L.tgnx_link_predictor_topk_ws_bytes(200, 9227, 100, 100, 1)


def test_reference_gives_tgb_ranks_against_negatives():
    """n_count = n_cand - 1, the target in the last row, no keys: the first n_cand - 1 columns are the negatives."""
    from link_rank_ref import link_rank_ref
    from oracle.mrr_ref import mrr_batch
    rng = np.random.default_rng(0)
    for trial in range(20):
        n_src, n_cand = int(rng.integers(1, 7)), int(rng.integers(2, 30))
        scores = rng.integers(-3, 4, (n_src, n_cand)).astype(np.float32)          # few values: many ties
        gt, eq, n, rank = link_rank_ref(scores, n_cand - 1, np.full(n_src, n_cand - 1))
        assert (n == n_cand - 1).all()
        for q in range(n_src):
            assert 1.0 / rank[q] == mrr_batch(scores[q, -1:], scores[q:q + 1, :-1]), (trial, q)


def test_reference_rules_on_hand_made_rows():
    from link_rank_ref import link_rank_ref
    nan = np.nan
    #                 0    1    2    3    4    5     6
    row = np.array([[2.0, 5.0, 2.0, nan, 1.0, 2.0, -0.0]], dtype=np.float32)
    # ties: target 0 (2.0) against 5.0 above, two more 2.0s; the NaN is compared nowhere
    gt, eq, n, rank = link_rank_ref(row, 7, [0])
    assert (gt[0], eq[0], n[0], rank[0]) == (1, 2, 5, 3.0)
    # float ==: -0 equals +0
    z = np.array([[0.0, -0.0, 1.0]], dtype=np.float32)
    assert [int(x[0]) for x in link_rank_ref(z, 3, [1])[:3]] == [1, 1, 2]
    # only the first n_count columns compete; a target past them is ranked against all of them
    gt, eq, n, rank = link_rank_ref(row, 4, [5])
    assert (gt[0], eq[0], n[0], rank[0]) == (1, 2, 3, 3.0)
    # duplicate keys: positions 2 and 5 carry the target's node and leave; position 1's node sits at 6 too
    key = np.array([7, 8, 7, 9, 10, 7, 8])
    gt, eq, n, rank = link_rank_ref(row, 7, [0], cand_key=key)
    assert (gt[0], eq[0], n[0], rank[0]) == (1, 0, 3, 2.0)
    # src_key removes node 8 at both positions; the exclusion list removes node 10, and naming the target's own key
    # (7) changes nothing: the target is never excluded
    gt, eq, n, rank = link_rank_ref(row, 7, [0], cand_key=key, src_key=[8])
    assert (gt[0], eq[0], n[0], rank[0]) == (0, 0, 1, 1.0)
    a = link_rank_ref(row, 7, [0], cand_key=key, excl_ptr=[0, 2], excl_key=[7, 10])
    assert (a[0][0], a[1][0], a[2][0], a[3][0]) == (1, 0, 2, 2.0)
    # everything excluded: n = 0, rank 1
    a = link_rank_ref(row, 7, [0], cand_key=key, excl_ptr=[0, 3], excl_key=[8, 9, 10])
    assert (a[0][0], a[1][0], a[2][0], a[3][0]) == (0, 0, 0, 1.0)
    # skipped rows: a NaN target logit, a target outside the matrix (the key rule is vacuous: all six non-NaN count)
    for t, want_n in ((3, 6), (-1, 6), (7, 6)):
        gt, eq, n, rank = link_rank_ref(row, 7, [t])
        assert gt[0] == 0 and eq[0] == 0 and n[0] == want_n and np.isnan(rank[0]), t
