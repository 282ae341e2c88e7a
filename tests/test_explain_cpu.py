"""CPU checks of the explanation surface (tgnx_tgn_explain, tgnx_link_predictor_loo and what sits on them): the two
references of explain_ref.py agree with each other on the state the GPU tests use, that state carries what the GPU
tests need (empty, single-slot, partial and full ring rows, repeated neighbours, effects far above the tolerance), the
library exports the entry points under the header's argument lists, the Python surface exists, and the argument checks
— explain()'s and ops.link_loo's (the ops layer has no CPU fallback: shapes only) — hold without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import explain_ref as xr
from conftest import ROOT

_STATE = {}


def _state(D=32, ring=10):
    if (D, ring) not in _STATE:
        s = xr.stream()
        ref, lref = xr.new_oracle(D, ring)
        ev_t, ev_msg = xr.advance(ref, lref, s, xr.negatives(s))
        _STATE[(D, ring)] = (s, ref, lref, ev_t, ev_msg)
    return _STATE[(D, ring)]


def test_the_state_has_every_kind_of_ring_row_and_effects_above_the_tolerance():
    s, ref, lref, ev_t, ev_msg = _state()
    src, dst = xr.pairs(s)
    cs, cd = (lref.e_id[src] >= 0).sum(1), (lref.e_id[dst] >= 0).sum(1)
    print("source ring counts", dict(zip(*np.unique(cs, return_counts=True))))
    print("destination ring counts", dict(zip(*np.unique(cd, return_counts=True))))
    assert (cs == 0).any() and (cs == 10).any() and ((cs > 0) & (cs < 10)).any()
    assert (cd == 1).any() and ((cd > 1) & (cd < 10)).any()
    rep = sum(len(set(lref.neighbors[v][lref.e_id[v] >= 0].tolist())) < c for v, c in zip(src, cs))
    print("source rows naming a neighbour twice:", rep)
    assert rep > 0
    want = xr.structural_explain(ref, lref, ev_t, ev_msg, src, dst, "slot")
    eff = np.abs(np.array([e for row in want["src"] for e in row.values()]))
    print(f"{eff.size} source-side slot effects: median {np.median(eff):.3e} max {eff.max():.3e}")
    assert eff.size == int(cs.sum()) and np.median(eff) > 1e-3          # > 25 x the 4e-5 the GPU test allows


@pytest.mark.parametrize("by", ["slot", "neighbour"])
def test_closed_form_equals_the_structural_reference(by):
    """float64 closed form against the float32 oracle forward with the slots masked out of the sampler.  The bound is
    the float32 side's rounding: values of magnitude ~1 from chained contractions of D + d = 48 and D = 32 terms, each
    term rounded to 2^-24 relative — 80 x 6e-8 = 5e-6 if every rounding went one way."""
    s, ref, lref, ev_t, ev_msg = _state()
    src, dst = xr.pairs(s)
    nodes = np.unique(np.concatenate([src, dst]))
    att = xr.oracle_attention(ref, lref, ev_t, ev_msg, nodes)
    worst = dict(z=0.0, loo=0.0, alpha=0.0)
    for v in nodes:
        a = xr.structural_node(ref, lref, ev_t, ev_msg, v, by)
        b = xr.closed_form_node(ref, lref, ev_t, ev_msg, v, by)
        assert b["loo_z"].shape == tuple(a["loo_z"].shape)
        worst["z"] = max(worst["z"], float(np.abs(a["z"].double().numpy() - b["z"]).max()))
        if a["event"].size:
            worst["loo"] = max(worst["loo"], float(np.abs(a["loo_z"].double().numpy() - b["loo_z"]).max()))
            al = np.stack([att[int(v)][int(e)] for e in a["event"]])
            worst["alpha"] = max(worst["alpha"], float(np.abs(al - b["alpha"]).max()))
            assert np.abs(b["alpha"].sum(0) - 1).max() < 1e-9
    print(worst)
    assert max(worst.values()) <= 5e-6, worst


def test_neighbour_mode_groups_repeat_interactions():
    s, ref, lref, ev_t, ev_msg = _state()
    src, _ = xr.pairs(s)
    for v in np.unique(src):
        pos, sets = xr.slot_sets(lref, v, "neighbour")
        nb = lref.neighbors[v][pos]
        for j, S in enumerate(sets):
            assert set(lref.neighbors[v][S].tolist()) == {nb[j]} and (nb == nb[j]).sum() == S.size
        a = xr.structural_node(ref, lref, ev_t, ev_msg, v, "neighbour")
        assert a["lead"].sum() == np.unique(nb).size
        for j in range(pos.size):     # every slot of a group carries the group's row
            first = int(np.flatnonzero(nb == nb[j])[0])
            assert torch.equal(a["loo_z"][j], a["loo_z"][first])


def test_single_slot_removed_is_the_embedding_of_an_empty_row():
    s, ref, lref, ev_t, ev_msg = _state()
    src, dst = xr.pairs(s)
    nodes = np.unique(np.concatenate([src, dst]))
    one = [v for v in nodes if (lref.e_id[v] >= 0).sum() == 1]
    assert one
    conv = ref.gnn.conv
    for v in one:
        a = xr.structural_node(ref, lref, ev_t, ev_msg, v, "slot")
        with torch.no_grad():
            skip = conv.lin_skip(ref.memory.memory[int(v)])
        assert float((a["loo_z"][0] - skip).abs().max()) <= 1e-6


# ---------------------------------------------------------------------------------------- the surface, without a device
def _decl(name):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tgnx.h")).read(), flags=re.S)
    m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


@pytest.mark.parametrize("name", ["tgnx_tgn_explain", "tgnx_link_predictor_loo", "tgnx_link_predictor_loo_ws_bytes"])
def test_library_exports_and_binds_the_entry_points(name):
    from tgnx import _lib
    assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    rtype, decl = _decl(name)
    assert (rtype == "int") == (res is ctypes.c_int) and len(decl) == len(args)
    for a, t in zip(decl, args):
        assert ("*" in a) == (t in (_lib.P, ctypes.c_void_p)), (name, a)


def test_python_surface_exists():
    import pyg_epoch_utils
    from tgnx import nn, ops, tgn_epoch
    from tgnx.tgn import TgnEngine
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(TgnEngine.attention) == ["self", "nodes", "validate"]
    assert inspect.signature(TgnEngine.attention).parameters["validate"].default is True
    assert par(TgnEngine.explain) == ["self", "src", "dst", "by"]
    assert inspect.signature(TgnEngine.explain).parameters["by"].default == "slot"
    assert par(tgn_epoch.explain) == ["model", "src", "dst", "by"]
    assert par(tgn_epoch.explain_recommendations)[:3] == ["model", "src", "k"]
    assert pyg_epoch_utils.explain is tgn_epoch.explain
    assert pyg_epoch_utils.explain_recommendations is tgn_epoch.explain_recommendations
    assert par(ops.link_loo) == ["z", "loo_z", "count", "src_row", "dst_row", "w_src", "b_src", "w_dst", "b_dst", "w_out",
                                 "b_out"]
    assert par(nn.LinkPredictor.loo) == ["self", "z", "loo_z", "count", "src_row", "dst_row"]
    assert "predictor_loo" in ops.OPS


def test_explain_argument_checks():
    from tgnx.tgn import check_explain_args
    assert check_explain_args("slot", 5, 5) == 0 and check_explain_args("neighbour", 0, 0) == 1
    with pytest.raises(ValueError, match="by"):
        check_explain_args("edge", 5, 5)
    with pytest.raises(ValueError, match="by"):
        check_explain_args(None, 5, 5)
    with pytest.raises(ValueError, match="5 sources for 4"):
        check_explain_args("slot", 5, 4)
    with pytest.raises(NotImplementedError, match="layers"):
        check_explain_args("slot", 5, 5, layers=2)
    with pytest.raises(NotImplementedError, match="world"):
        check_explain_args("slot", 5, 5, world=2)


def test_explain_refuses_on_a_stub_engine_before_any_device_call():
    """TgnEngine.explain on a stub that has only what the checks read: it must raise before it embeds anything."""
    from tgnx.tgn import TgnEngine

    class Cfg:
        layers, num_nodes, ring, mem_dim = 1, 300, 10, 32

    class Stub:
        cfg, world, dev = Cfg(), 1, torch.device("cpu")
        _ids = TgnEngine._ids

        def _explain_nodes(self, *a, **k):
            raise AssertionError("reached the device")

    stub = Stub()
    with pytest.raises(ValueError, match="by"):
        TgnEngine.explain(stub, [1, 2], [3, 4], by="node")
    with pytest.raises(ValueError, match="sources"):
        TgnEngine.explain(stub, [1, 2], [3], by="slot")
    with pytest.raises(ValueError, match="node ids"):
        TgnEngine.explain(stub, [1, 300], [3, 4])
    stub.world = 2
    with pytest.raises(NotImplementedError):
        TgnEngine.explain(stub, [1, 2], [3, 4])
    stub.world, stub.cfg.layers = 1, 2
    with pytest.raises(NotImplementedError):
        TgnEngine.explain(stub, [1, 2], [3, 4])


def test_link_loo_shape_checks():
    from tgnx.ops import check_link_loo_args
    assert check_link_loo_args((7, 32), (7, 3, 32), 7, 13, 13) == (7, 3, 13)
    assert check_link_loo_args((0, 32), (0, 3, 32), 0, 0, 0) == (0, 3, 0)
    for bad in (((7, 32), (7, 3, 31), 7, 13, 13), ((7, 32), (6, 3, 32), 7, 13, 13), ((7, 32), (7, 32), 7, 13, 13),
                ((7, 32), (7, 0, 32), 7, 13, 13), ((7, 32), (7, 65, 32), 7, 13, 13), ((7, 32), (7, 3, 32), 6, 13, 13),
                ((7, 32), (7, 3, 32), 7, 13, 12)):
        with pytest.raises(ValueError, match="link_loo"):
            check_link_loo_args(*bad)


def test_c_entries_check_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers, TgnConfig
    L = _lib.lib()
    keep = np.zeros(4096, dtype=np.float32)
    p, null = ctypes.c_void_p(keep.ctypes.data), ctypes.c_void_p(0)
    failed = lambda rc: rc == -1 and len(L.tgnx_last_error()) > 0  # noqa: E731  (TGNX_EINVAL)
    cfg = dict(num_nodes=300, num_events=600, ring=10, mem_dim=32, msg_dim=16, heads=2, max_batch=8, max_neg=1, aggr=0,
               dropout=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, layers=1, updater=0, emb_in_msg=0)
    b = TgnBuffers()
    for f, _ in TgnBuffers._fields_:
        if f not in ("n_dst", "xcap", "flags", "xrows", "plan_table", "out_ev", "neg", "out_pos", "out_neg", "mrr"):
            setattr(b, f, p.value)
    ex = lambda c, n, mode, loo, bufs=b: L.tgnx_tgn_explain(  # noqa: E731
        ctypes.byref(TgnConfig(**c)), ctypes.byref(bufs), p, n, mode, p, p, p, p, p, loo, null, null)
    assert failed(ex(cfg, 4, 2, p)) and b"mode" in L.tgnx_last_error()
    assert failed(ex(cfg, 25, 0, p)) and b"tgnx_tgn_embed_max_nodes" in L.tgnx_last_error()       # capacity 24
    assert failed(ex(dict(cfg, layers=2), 4, 0, p)) and b"layers = 1" in L.tgnx_last_error()      # loo_z at 2 hops
    assert failed(ex(dict(cfg, ring=0), 4, 0, p))
    assert failed(L.tgnx_tgn_explain(ctypes.byref(TgnConfig(**cfg)), ctypes.byref(b), p, 4, 0, null, p, p, p, p, p, null,
                                     null))
    assert ex(cfg, 0, 0, p) == 0                                                                  # n = 0: nothing
    loo = lambda n, K, P, D, ws_bytes, z=p: L.tgnx_link_predictor_loo(  # noqa: E731
        n, K, P, D, D, z, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, ws_bytes, null)
    big = L.tgnx_link_predictor_loo_ws_bytes(7, 3, 13, 32, 32)
    assert big > 4 * 7 * 4 * 32 * 4 // 2
    assert failed(loo(7, 0, 13, 32, big)) and failed(loo(7, 65, 13, 32, big)) and failed(loo(7, 3, 13, 257, big))
    assert failed(loo(7, 3, 13, 32, big - 1)) and b"workspace" in L.tgnx_last_error()
    assert failed(loo(7, 3, 13, 32, big, z=null))
    assert loo(7, 3, 0, 32, big) == 0                                                             # P = 0: nothing
    assert keep.sum() == 0
