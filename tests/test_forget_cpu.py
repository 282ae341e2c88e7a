"""CPU checks of forgetting nodes: the numpy restatement (tests/forget_ref.py) on a hand-written
state with literal expectations and on simulated streams (a node in nobody's ring, a node in every ring, a removal
that empties a run, every node, duplicates, the hub whose runs span several 64-entry chunks); the restatement applied
to the oracle (memory, message stores, loader) against an oracle that never saw the forgotten component, with batches
observed afterwards; the host argument check; the Python and C surface with its keyword defaults; the C calls'
argument checks on host pointers (nothing is launched, nothing is touched)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from compact_ref import deref
from conftest import ROOT
from embtab_ref import oracle_observe
from forget_ref import (component_events, forget_ref, hub_events, make_events, names_forgotten, oracle_forget,
                        ring_forget, simulate)
from test_compact_cpu import _tgn_cfg
from tgn_oracle_steps import MEM_TOL

NAMES = {"tgnx_tgn_forget_ws_bytes": ("size_t", 1), "tgnx_tgn_forget_plan": ("int", 8),
         "tgnx_tgn_forget_apply": ("int", 7), "tgnx_ring_forget": ("int", 12)}
I, F32 = np.int64, np.float32


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(_bits(np.asarray(a[k])), _bits(np.asarray(b[k]))), k


# ---------------------------------------------------------------------------------------------- the restatement
def _hand():
    """N = 4, K = 3, six events.  Node 1 is in the rings of 0 and 2 and at the other end of entries of both stores."""
    src, dst = np.array([0, 1, 2, 0, 1, 3], I), np.array([1, 2, 0, 2, 0, 3], I)
    t = np.array([5, 9, 9, 9, 12, 12], F32)          # event 4 (0 <- 1) is newer than event 3 (0 -> 2)
    nbr = np.array([[1, 2, 2], [0, 2, 0], [0, 0, 1], [3, 7, -1]], I)       # row 3: one valid slot, a stale id, -1
    eid = np.array([[4, 3, 2], [4, 1, 0], [3, 2, 1], [5, -1, -1]], I)
    rt = np.array([[12, 9, 9], [12, 9, 5], [9, 9, 9], [12, -1, -1]], F32)
    #        s run        d run
    nodes = np.array([[0, 1, 2, 2], [4, 2, 6, 1], [7, 1, 8, 2], [10, 1, 11, 1]], I)
    arena = np.array([3, -7, 2, 4, 1, 4, 0, 2, 1, 3, 5, 5], I)     # (word 1 belongs to nobody)
    return dict(nbr=nbr, eid=eid, rt=rt, nodes=nodes, arena=arena, src=src, dst=dst, t=t,
                memory=np.arange(8, dtype=F32).reshape(4, 2) + 1, last_update=np.array([12, 12, 9, 12], I),
                node_gen=np.array([3, 3, 2, 3], np.int32))


def test_restatement_on_a_hand_written_state():
    h = _hand()
    h0 = {k: v.copy() for k, v in h.items()}
    g, counts = forget_ref(h, [1])
    _same(h, h0)                                                         # the input is not written
    assert counts == dict(nodes=1, ring_slots=2, ring_rows=2, store_entries=2)
    assert g["nbr"].tolist() == [[2, 2, -1], [-1, -1, -1], [0, 0, -1], [3, 7, -1]]      # row 3 keeps its stale id
    assert g["eid"].tolist() == [[3, 2, -1], [-1, -1, -1], [3, 2, -1], [5, -1, -1]]
    assert g["rt"].tolist() == [[9, 9, -1], [-1, -1, -1], [9, 9, -1], [12, -1, -1]]
    # node 0: s run [3] keeps (dst 2); d run [2, 4] loses 4 (src 1).  node 2: s run [2] (dst 0) stays; d run [1, 3]
    # loses 1 (src 1).  node 1: reset.  node 3: untouched
    assert g["nodes"].tolist() == [[0, 1, 2, 1], [0, 0, 0, 0], [7, 1, 8, 1], [10, 1, 11, 1]]
    assert g["arena"].tolist() == [3, -7, 2, 4, 1, 4, 0, 2, 3, 3, 5, 5]   # packed in place; the tails keep old words
    assert g["memory"].tolist() == [[1, 2], [0, 0], [5, 6], [7, 8]]
    assert g["last_update"].tolist() == [12, 0, 9, 12] and g["node_gen"].tolist() == [3, 0, 2, 3]
    assert not names_forgotten(g, [1]) and names_forgotten(h, [1])
    # a removal that empties a run: forgetting 0 empties node 2's s run {7, 1} -> {0, 0}
    g0, c0 = forget_ref(h, [0])
    assert g0["nodes"][2].tolist() == [0, 0, 8, 1] and g0["arena"][8] == 1 and c0["store_entries"] == 4     # 1: {4}, {0}; 2: {2}, {3}
    # the t column is re-ranked from the table: a shuffled-t ring row is repaired to the kept events' times
    h2 = _hand()
    h2["t"] = np.array([5, 9, 30, 9, 12, 12], F32)                        # event 2 now has the largest t
    g2, _ = forget_ref(h2, [1])
    assert g2["rt"][0].tolist() == [30, 9, -1] and g2["eid"][0].tolist() == [3, 2, -1]
    n2, e2, t2, c2 = ring_forget(h2["nbr"], h2["eid"], h2["rt"], [1])     # a loader alone: the slots e_id drops
    assert t2[0].tolist() == [9, 9, -1] and np.array_equal(e2, g2["eid"]) and np.array_equal(n2, g2["nbr"])
    assert c2 == dict(nodes=1, ring_slots=2, ring_rows=2)
    for bad in ([4], [-1], [0, 9]):
        with pytest.raises(ValueError, match="node ids"):
            forget_ref(h, bad)


N_SIM, K_SIM, B_SIM = 70, 4, 50


def _sim():
    ev = make_events(3, 600, N_SIM - 2, 5)                # nodes 68, 69 never occur
    ev["src"][-68:], ev["dst"][-68:] = 11, np.arange(68)  # node 11 ends by talking to everybody: it is in every ring
    return ev, simulate(ev, B_SIM, N_SIM, K_SIM)


def _untouched_rows_keep_their_bits(h, g, ids):
    inF = np.zeros(h["nbr"].shape[0], bool)
    inF[np.asarray(ids)] = True
    valid = (h["eid"] >= 0) & (h["nbr"] != -1)
    hit = np.zeros_like(valid)
    hit[valid] = inF[h["nbr"][valid]]
    quiet = ~inF & ~hit.any(1)
    for k in ("nbr", "eid", "rt"):
        assert np.array_equal(_bits(g[k][quiet]), _bits(h[k][quiet])), k
    for k in ("memory", "last_update", "node_gen"):
        assert np.array_equal(_bits(g[k][~inF]), _bits(h[k][~inF])), k
    assert np.array_equal(g["nodes"][~inF][:, [0, 2]][g["nodes"][~inF][:, [1, 3]] > 0],
                          h["nodes"][~inF][:, [0, 2]][g["nodes"][~inF][:, [1, 3]] > 0])     # offsets stay
    return int(quiet.sum())


def test_restatement_on_simulated_streams():
    ev, h = _sim()
    h["memory"] = np.random.default_rng(0).standard_normal((N_SIM, 4)).astype(F32)
    h["last_update"], h["node_gen"] = np.arange(N_SIM, dtype=I) + 1, np.arange(N_SIM, dtype=np.int32) + 1
    # a node in nobody's ring: only its own (already empty) rows
    g, c = forget_ref(h, [69])
    assert c == dict(nodes=1, ring_slots=0, ring_rows=0, store_entries=0)
    _same(g, h, ("nbr", "eid", "rt", "nodes", "arena"))
    assert g["memory"][69].tolist() == [0] * 4 and g["last_update"][69] == 0 and g["node_gen"][69] == 0
    # a node in every ring
    g, c = forget_ref(h, [11])
    assert c["ring_rows"] == 67 and c["ring_slots"] >= c["ring_rows"] and c["store_entries"] > 0
    assert not names_forgotten(g, [11]) and names_forgotten(h, [11])
    assert _untouched_rows_keep_their_bits(h, g, [11]) >= 2
    valid = g["eid"] >= 0
    assert np.all(np.diff(np.where(valid, g["eid"], -1), axis=1) <= 0)           # e_id stays ranked descending
    assert np.all(np.diff(g["rt"], axis=1) <= 0) and np.all(valid == (g["nbr"] != -1))
    assert np.array_equal(g["rt"][valid], h["t"][g["eid"][valid]])               # time-ordered: the same slots dropped
    # several nodes, with duplicates: the same result and the distinct count
    ids = [11, 3, 0, 69, 3, 11, 11]
    g1, c1 = forget_ref(h, ids)
    g2, c2 = forget_ref(h, sorted(set(ids)))
    _same(g1, g2)
    assert c1 == c2 and c1["nodes"] == 4 and not names_forgotten(g1, ids)
    assert _untouched_rows_keep_their_bits(h, g1, sorted(set(ids))) >= 1
    # forgetting in two calls equals forgetting at once (the state, not the counts)
    g3, _ = forget_ref(forget_ref(h, [11, 3])[0], [0, 69])
    _same(g3, g1, ("nbr", "eid", "rt", "nodes", "memory", "last_update", "node_gen"))
    _same(deref(g3), deref(g1))
    # every node: a reset ring and empty stores
    ga, ca = forget_ref(h, np.arange(N_SIM))
    assert ca == dict(nodes=N_SIM, ring_slots=0, ring_rows=0, store_entries=0)
    assert (ga["nbr"] == -1).all() and (ga["eid"] == -1).all() and (ga["rt"] == -1).all()
    assert not ga["nodes"].any() and not ga["memory"].any() and np.array_equal(ga["arena"], h["arena"])
    # an empty list: nothing
    ge, ce = forget_ref(h, [])
    _same(ge, h)
    assert ce == dict(nodes=0, ring_slots=0, ring_rows=0, store_entries=0)


def test_restatement_on_the_hub():
    hub, B = 7, 200
    ev = hub_events(4, N_SIM, 5, hub=hub, B=B)
    h = simulate(ev, B, N_SIM, 10)
    assert h["nodes"][hub].tolist()[1::2] == [150, 70]                # three and two 64-entry chunks
    # the hub as the partner: forget a third of the nodes, the hub's runs are packed across chunk boundaries
    ids = np.arange(10, N_SIM, 3)
    g, c = forget_ref(h, ids)
    s_run = h["arena"][h["nodes"][hub, 0]:][:150]
    keep = s_run[~np.isin(h["dst"][s_run], ids)]
    assert 64 < keep.size < 150 and g["nodes"][hub, 1] == keep.size and g["nodes"][hub, 0] == h["nodes"][hub, 0]
    assert np.array_equal(g["arena"][g["nodes"][hub, 0]:][:keep.size], keep) and not names_forgotten(g, ids)
    # the hub forgotten: every node it talked to in the last batch loses an entry, its self loops go with its row
    g, c = forget_ref(h, [hub])
    assert g["nodes"][hub].tolist() == [0, 0, 0, 0] and not names_forgotten(g, [hub])
    assert c["store_entries"] == 130 + 50                              # 150 + 70 entries less the 20 self loops, twice


# ---------------------------------------------------------------------------------------------- the oracle
def _oracle(N, d, D=32, ring=4):
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN
    torch.manual_seed(0)
    ref = RefTGN(N, d, hidden=D, dropout=0.0)
    ref.memory.reset_state()
    ref.eval()
    return ref, RefLastNeighborLoader(N, ring)


class _S:            # (oracle_observe reads s.src / s.dst)
    def __init__(self, ev):
        self.src, self.dst = ev["src"], ev["dst"]


def _store_rows(store, u):
    return [x.numpy().copy() for x in store[u][1:]] if u in store else None


def test_restatement_applied_to_the_oracle_equals_an_oracle_that_never_saw_the_component():
    """The stream of the GPU twin test on the CPU: nodes [60, 70) interact among themselves only.  Oracle A observes
    everything and forgets them; oracle B observes the same batches without their events.  On [0, 60): loader rows
    equal through the event rows they name, stores equal (partner, t, raw), memory within MEM_TOL — and the same after
    three more batches on both sides."""
    N, d, B, nev, more = 70, 5, 50, 600, 150
    ev, comp = component_events(8, nev + more, d)
    assert 60 < comp[:nev].sum() < 200 and comp[:B].any()
    t, msg = torch.from_numpy(ev["t"]), torch.from_numpy(ev["msg"])
    (a, la), (b, lb) = _oracle(N, d), _oracle(N, d)
    b.load_state_dict(a.state_dict())
    b.memory._reset_message_store()
    sub = {k: v[~comp] for k, v in ev.items()}                     # B's table: the main component's rows, renumbered
    tb, msgb = torch.from_numpy(sub["t"]), torch.from_numpy(sub["msg"])
    new_id = np.cumsum(~comp) - 1

    def observe_both(lo, hi):
        for s in range(lo, hi, B):
            oracle_observe(a, la, _S(ev), t, msg, s, s + B)
            keep = np.flatnonzero(~comp[s:s + B]) + s
            oracle_observe(b, lb, _S(sub), tb, msgb, int(new_id[keep[0]]), int(new_id[keep[-1]]) + 1)

    def compare():
        va = la.e_id[:60] >= 0
        assert np.array_equal(va, lb.e_id[:60] >= 0) and np.array_equal(la.neighbors[:60][va], lb.neighbors[:60][va])
        assert np.array_equal(new_id[la.e_id[:60][va]], lb.e_id[:60][va])
        assert np.array_equal(_bits(la.t[:60]), _bits(lb.t[:60]))
        for sa, sb in ((a.memory.msg_s_store, b.memory.msg_s_store), (a.memory.msg_d_store, b.memory.msg_d_store)):
            assert sorted(sa) == sorted(sb) and all(u < 60 for u in sa)
            for u in sa:
                for x, y in zip(_store_rows(sa, u), _store_rows(sb, u)):
                    assert np.array_equal(_bits(x), _bits(y)), u
        err = float((a.memory.memory[:60] - b.memory.memory[:60]).abs().max())
        print(f"memory [0, 60): max err {err:.3e} (bound {MEM_TOL:.1e})")
        assert err <= MEM_TOL
        assert torch.equal(a.memory.last_update[:60], b.memory.last_update[:60])
        assert (la.e_id[60:] == -1).all() and (la.neighbors[60:] == -1).all() and (la.t[60:] == -1).all()
        assert not a.memory.memory[60:].any() and not a.memory.last_update[60:].any()

    observe_both(0, nev)
    before = dict(mem=a.memory.memory.clone(), lu=a.memory.last_update.clone(), nbr=la.neighbors.copy(),
                  eid=la.e_id.copy(), t=la.t.copy(),
                  s={u: _store_rows(a.memory.msg_s_store, u) for u in range(N)},
                  d={u: _store_rows(a.memory.msg_d_store, u) for u in range(N)})
    assert (la.e_id[60:] >= 0).any() and a.memory.memory[60:].any()
    oracle_forget(a, la, np.arange(60, 70), ev["t"])
    # no row of [0, 60) named the component: every one is exactly unchanged
    assert torch.equal(a.memory.memory[:60], before["mem"][:60]) and torch.equal(a.memory.last_update[:60], before["lu"][:60])
    for k, x in (("nbr", la.neighbors), ("eid", la.e_id), ("t", la.t)):
        assert np.array_equal(_bits(x[:60]), _bits(before[k][:60])), k
    for key, st in (("s", a.memory.msg_s_store), ("d", a.memory.msg_d_store)):
        for u in range(60):
            x, y = _store_rows(st, u), before[key][u]
            assert (x is None) == (y is None) and (x is None or all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x, y)))
    compare()
    observe_both(nev, nev + more)
    assert (la.e_id[60:] >= 0).any()                           # the forgotten ids are observed again: an id reused
    oracle_forget(a, la, np.arange(60, 70), ev["t"])
    compare()


def test_restatement_applied_to_the_oracle_removes_partners():
    """A forgotten node with partners: rows that named it lose exactly those entries, every other row is unchanged."""
    N, d, B = 40, 5, 50
    ev = make_events(2, 300, N, d)
    t, msg = torch.from_numpy(ev["t"]), torch.from_numpy(ev["msg"])
    a, la = _oracle(N, d)
    for s in range(0, 300, B):
        oracle_observe(a, la, _S(ev), t, msg, s, s + B)
    F = [5, 17]
    s0 = {u: _store_rows(a.memory.msg_s_store, u) for u in range(N)}
    nbr0, eid0, t0, mem0 = la.neighbors.copy(), la.e_id.copy(), la.t.copy(), a.memory.memory.clone()
    oracle_forget(a, la, F, ev["t"])
    named = np.isin(nbr0, F).any(1)
    assert named.sum() > 2 and (~named).sum() > 2
    for u in range(N):
        if u in F:
            assert (la.e_id[u] == -1).all() and not a.memory.memory[u].any() and u not in a.memory.msg_s_store
            continue
        assert torch.equal(a.memory.memory[u], mem0[u])
        if not named[u]:
            assert np.array_equal(la.neighbors[u], nbr0[u]) and np.array_equal(la.e_id[u], eid0[u])
            assert np.array_equal(_bits(la.t[u]), _bits(t0[u]))
        else:
            keep = ~np.isin(nbr0[u], F) & (eid0[u] >= 0)
            assert np.array_equal(la.e_id[u][:keep.sum()], eid0[u][keep]) and (la.e_id[u][keep.sum():] == -1).all()
        rows = _store_rows(a.memory.msg_s_store, u)
        if s0[u] is not None:
            keep = ~np.isin(s0[u][0], F)
            assert (rows is None) == (not keep.any())
            assert rows is None or all(np.array_equal(_bits(x), _bits(y[keep])) for x, y in zip(rows, s0[u]))
    # and the oracle goes on
    ev2 = make_events(9, B, N, d)
    ev2["t"] += ev["t"][-1]
    oracle_observe(a, la, _S(ev2), torch.from_numpy(ev2["t"]), torch.from_numpy(ev2["msg"]), 0, B)
    assert torch.isfinite(a.memory.memory).all()


# ---------------------------------------------------------------------------------------------- host checks, surface
def test_check_forget_args():
    from tgnx.tgn import FORGET_COUNTS, check_forget_args
    assert FORGET_COUNTS == ("nodes", "ring_slots", "ring_rows", "store_entries")
    assert check_forget_args(300, 1) is True and check_forget_args(1, 5000) is True
    assert check_forget_args(300, 0) is False                              # an empty list: nothing to do
    assert check_forget_args(300, 3, world=1, dp=False) is True
    for kw in (dict(world=2), dict(dp=True), dict(world=8, dp=True)):
        with pytest.raises(ValueError, match="one device"):
            check_forget_args(300, 3, **kw)
        with pytest.raises(ValueError, match="one device"):
            check_forget_args(300, 0, **kw)                                # refused before the empty list is a no-op
    with pytest.raises(ValueError, match="num_nodes"):
        check_forget_args(0, 3)
    for n in (-1, 1 << 31):
        with pytest.raises(ValueError, match="ids"):
            check_forget_args(300, n)


def test_python_surface_and_keyword_defaults():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnEngine
    sig = inspect.signature(TgnEngine.forget_nodes)
    assert list(sig.parameters) == ["self", "ids", "compact", "drop_candidates"]
    for k in ("compact", "drop_candidates"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is False
    assert list(inspect.signature(LastNeighborLoader.forget).parameters) == ["self", "ids"]
    sig = inspect.signature(tgn_epoch.forget)
    assert list(sig.parameters) == ["model", "neighbor_loader", "ids", "compact", "drop_candidates"]
    assert sig.parameters["compact"].default is False and sig.parameters["drop_candidates"].default is False
    assert pyg_epoch_utils.forget is tgn_epoch.forget
    doc = TgnEngine.forget_nodes.__doc__
    for word in ("NOT undone", "drop_candidates", "not observed yet", "shuffled"):
        assert word in doc, word
    # no checkpoint format change, and the entry points other tests pin keep their lists
    from tgnx.tgn import STREAM_STATE_FORMAT
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert STREAM_STATE_FORMAT == 1 and par(TgnEngine.compact_events) == ["self", "upto", "capacity"]
    assert par(TgnEngine.grow_nodes) == ["self", "n"] and par(TgnEngine.load_stream_state) == ["self", "state"]


def test_header_declares_and_library_exports_the_entry_points():
    from tgnx import _lib
    raw = open(os.path.join(ROOT, "include", "tgnx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    decls = {}
    for name, (res, nargs) in NAMES.items():
        m = re.search(r"([A-Za-z0-9_]+)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m and m.group(1) == res, name
        decls[name] = [a.strip() for a in m.group(2).split(",")]
        assert len(decls[name]) == nargs and name in _lib.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "tgb-tgn-dgl_amd", "csrc", "tgnx_forget.hip"))
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtgnx.so is not built here")
    L = _lib.lib()
    for name, decl in decls.items():
        assert hasattr(L, name)
        rtype, args = _lib.SIGNATURES[name]
        assert len(args) == len(decl)
        for a, c in zip(decl, args):
            assert ("*" in a) == (c is _lib.P), (name, a)
            assert not a.startswith("int64_t ") or c is ctypes.c_int64, (name, a)


def test_c_calls_check_arguments_before_any_device_call():
    from tgnx import _lib
    from tgnx.tgn import TgnBuffers
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtgnx.so is not built here")
    L = _lib.lib()
    cfg = _tgn_cfg()
    nb = int(L.tgnx_tgn_forget_ws_bytes(ctypes.byref(cfg)))
    assert nb == 64 + 48 + 304                           # record, 10 bitmap words and 300 bytes, each padded to 16
    assert L.tgnx_tgn_forget_ws_bytes(None) == 0 and L.tgnx_tgn_forget_ws_bytes(ctypes.byref(_tgn_cfg(num_nodes=0))) == 0
    assert L.tgnx_tgn_forget_ws_bytes(ctypes.byref(_tgn_cfg(num_nodes=1 << 31))) == 0
    keep = np.zeros(4096, dtype=np.float32)              # host memory: must never be touched
    p = ctypes.c_void_p(keep.ctypes.data)
    null = ctypes.c_void_p(0)
    need = ("nbr", "eid", "rt", "store", "ev_src", "ev_dst", "ev_t", "memory", "last_update", "node_gen")

    def bufs(*zero, **extra):
        b = TgnBuffers()
        for f in need:
            setattr(b, f, 0 if f in zero else p.value)
        for f, v in extra.items():
            setattr(b, f, v)
        return b

    def plan(cfg_ref=None, b=None, nev=600, ids=p, n=3, ws=p, ws_bytes=nb):
        return L.tgnx_tgn_forget_plan(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                      ctypes.byref(bufs()) if b is None else b, nev, ids, n, ws, ws_bytes, null)

    def apply(cfg_ref=None, b=None, nev=600, ws=p, ws_bytes=nb, **_):
        return L.tgnx_tgn_forget_apply(ctypes.byref(cfg) if cfg_ref is None else cfg_ref,
                                       ctypes.byref(bufs()) if b is None else b, nev, ws, ws_bytes, null, null)

    def ring(nbr=p, eid=p, rt=p, N=300, K=10, ids=p, n=3, ws=p, ws_bytes=nb):
        return L.tgnx_ring_forget(nbr, eid, rt, null, 0, N, K, ids, n, ws, ws_bytes, null)

    def failed(rc, code=-1):
        return rc == code and len(L.tgnx_last_error()) > 0

    for f in (plan, apply):
        assert failed(f(cfg_ref=null)) and failed(f(b=null)) and failed(f(ws=null)) and failed(f(ws_bytes=nb - 16))
        assert f.__name__.encode() in L.tgnx_last_error()
        assert failed(f(ws=ctypes.c_void_p(p.value + 8)))                  # 16-B alignment
        assert failed(f(nev=-1)) and failed(f(nev=601))                    # valid rows within the capacity
        for bad in (dict(num_nodes=0), dict(ring=0), dict(ring=33), dict(num_events=0), dict(mem_dim=0)):
            assert failed(f(cfg_ref=ctypes.byref(_tgn_cfg(**bad)))), bad
        assert failed(f(cfg_ref=ctypes.byref(_tgn_cfg(num_nodes=1 << 31))), code=-3)
        for field in need:
            assert failed(f(b=ctypes.byref(bufs(field)))), field
        assert failed(f(b=ctypes.byref(bufs(xrows=p.value, xcap=4))))      # a data-parallel engine
    assert failed(plan(ids=null)) and failed(plan(n=-1)) and failed(plan(n=1 << 31))
    assert failed(ring(nbr=null)) and failed(ring(eid=null)) and failed(ring(rt=null)) and failed(ring(ids=null))
    assert failed(ring(N=0)) and failed(ring(K=0)) and failed(ring(K=33)) and failed(ring(N=1 << 31), code=-3)
    assert failed(ring(ws=null)) and failed(ring(ws_bytes=nb - 16)) and failed(ring(n=-1))
    assert keep.sum() == 0
