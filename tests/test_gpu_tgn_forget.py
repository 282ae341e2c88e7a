"""GPU tests of forgetting nodes: tgnx_tgn_forget_plan / _apply, tgnx_ring_forget, TgnEngine.forget_nodes,
LastNeighborLoader.forget and the drop-in forget.

Setup as in test_gpu_tgn_compact.py: parameters from a RefTGN state dict, dropout 0, engines reset and flushed, moved
by observe only, so comparisons against the numpy restatement (tests/forget_ref.py, applied to a host snapshot taken
before the call) are exact.  Shapes: N = 70 and 257 (the bitmap's tail word, the row-byte tail), ring 4 / 10 / 32
(16, 6 and 2 rows per wave), msg_dim 5 and 16, D = 32, B = 50; the hub stream at B = 200, where one node is the source
of 150 events and the destination of 70 (runs of three and two 64-entry chunks).

  exact        every state tensor bit for bit, the whole tensors, and the returned counts: a never-seen node, node 0,
               node N - 1, duplicates, a node in every ring (its removal empties runs), every node; the hub as partner
               and as F; six model forms; a shuffled-t stream; forgotten rows against rows grow_nodes adds; compaction
               afterwards;
  semantics    the component twin (an engine that never saw the forgotten component, existing code only), the oracle
               continuation, a train batch against a twin loaded from the forgotten state, the embedding table;
  lifecycle    bindings and graphs, the empty list, checkpoints, drop_candidates, a loader alone, the drop-in;
  refusals     an id >= N, a corrupted e_id: the engine is untouched bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from compact_ref import assert_same_deref, deref
from embtab_ref import oracle_observe, stale_ids
from forget_ref import component_events, forget_ref, hub_events, make_events, names_forgotten, oracle_forget, ring_forget
from tgn_oracle_steps import MEM_TOL, Rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
D, B, KN = 32, 50, 5
TOL = 2e-5
FORMS = {"1hop_last": dict(layers=1, aggr="last"), "1hop_mean": dict(layers=1, aggr="mean"),
         "2hop_last": dict(layers=2, aggr="last"), "2hop_mean": dict(layers=2, aggr="mean"),
         "rnn": dict(layers=1, aggr="last", updater="rnn"),
         "dyrep_emb": dict(layers=1, aggr="last", memory="dyrep", use_src_emb_in_msg=True)}
CTL = {"NB": 10, "ERR": 11}
STATE = ("nbr", "eid", "rt", "nodes", "arena", "memory", "last_update", "node_gen")
REST = ("src", "dst", "t", "msg", "ctl", "flat", "n", "cap")


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


_SD = {}


def _sd(form, N, d):
    from oracle.tgn_ref import RefTGN
    key = (form, N, d)
    if key not in _SD:
        kw = dict(FORMS[form])
        kw.pop("memory", None)
        torch.manual_seed(0)
        _SD[key] = RefTGN(N, d, hidden=D, dropout=0.0, **kw).state_dict()
    return _SD[key]


def _engine(ev, N, form="1hop_last", ring=10, max_batch=B, dst_nodes="all", flush=True, rows=None):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    d = ev["msg"].shape[1]
    n = ev["src"].shape[0] if rows is None else rows
    model = TGNModel(N, max(n, 1), d, D, DEV, ring=ring, max_batch=max_batch, max_neg=KN, dropout=0.0, **FORMS[form])
    model.load_reference_state(_sd(form, N, d))
    eng = TgnEngine(model, LastNeighborLoader(N, ring, device=DEV), {k: v[:max(n, 1)] for k, v in ev.items()},
                    TgnAdam(model, 1e-3), dst_nodes=np.arange(N) if isinstance(dst_nodes, str) else dst_nodes, seed=7)
    eng.reset_state()
    if flush:
        eng.flush()
    return eng


def _host(eng):
    torch.cuda.synchronize()
    m, ld, Nn = eng.model, eng.loader, eng.cfg.num_nodes
    st = m.store.cpu().numpy()
    g = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    return dict(n=eng.num_events, cap=eng.event_capacity, nbr=g(ld.neighbors), eid=g(ld.e_id), rt=g(ld.t),
                nodes=st[:4 * Nn].reshape(Nn, 4).copy(), arena=st[4 * Nn:].copy(), src=g(eng.src), dst=g(eng.dst),
                t=g(eng.t), msg=g(eng.msg), memory=g(m.memory.memory), last_update=g(m.memory.last_update),
                node_gen=g(m.node_gen), ctl=g(eng.ctl), flat=g(m.flat))


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x))
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _check_forget(eng, ids, **kw):
    """forget_nodes against the restatement on a snapshot taken before the call: every state tensor whole and bit for
    bit, nothing else moved, the counts.  Returns (before, after, counts)."""
    h0 = _host(eng)
    ver = eng.loader.version
    want, counts = forget_ref(h0, ids)
    got = eng.forget_nodes(ids, **kw)
    h1 = _host(eng)
    eng.check()
    print(f"forget {np.asarray(ids).reshape(-1)[:8].tolist()}...: {counts}")
    assert {k: got[k] for k in counts} == counts
    _same(h1, want, STATE)
    if not kw.get("compact"):
        _same(h1, h0, REST)
    assert eng.loader.version == ver + (1 if np.asarray(ids).size else 0)
    assert not names_forgotten(h1, ids) or kw.get("compact")
    return h0, h1, counts


def _popular_stream(N, d, nev=600):
    """Random events over [0, N - 2) (nodes N - 2, N - 1 never occur) that end with node 11 talking to 68 nodes, one
    event each: 11 is the newest entry of their rings and the only entry of their last d runs."""
    ev = make_events(3, nev, N - 2, d)
    ev["src"][-68:], ev["dst"][-68:] = 11, np.arange(68)
    return ev


# ---------------------------------------------------------------------------------------------- exact
def _exact_sequence(form, N, ring, d):
    ev = _popular_stream(N, d)
    e = _engine(ev, N, form, ring, flush=False)     # (a flush gives a never-seen node the row cell(0, 0): DESIGN §3b-8)
    e.observe_range(0, 600, B)
    # a never-seen node: all counts zero, nothing written
    h0, h1, c = _check_forget(e, [N - 1])
    assert c == dict(nodes=1, ring_slots=0, ring_rows=0, store_entries=0)
    _same(h1, h0, STATE)
    # node 0, then duplicates
    h0, h1, c = _check_forget(e, [0])
    assert c["ring_slots"] > 0 and c["store_entries"] > 0
    h0, h1, c = _check_forget(e, [5, 31, 5, 64, 31, 5])
    assert c["nodes"] == 3 and c["ring_rows"] > 0
    # the node in every ring: rows of the ring's every layout position lose their first slot, runs are emptied
    h0, h1, c = _check_forget(e, torch.tensor([11]))
    assert c["ring_rows"] >= 60 and c["ring_slots"] >= c["ring_rows"]
    emptied = (h0["nodes"][:, 3] > 0) & (h1["nodes"][:, 3] == 0) & (np.arange(N) != 11)
    assert emptied.sum() >= 30 and not h1["nodes"][emptied][:, 2].any()              # {off, cnt} = {0, 0}
    assert int((_bits(h0["rt"]) == _bits(h1["rt"])).all(1).sum()) >= 2               # some rows named nothing
    # every node (ids in descending order, with a duplicate)
    h0, h1, c = _check_forget(e, np.concatenate([np.arange(N)[::-1], [3]]))
    assert c == dict(nodes=N, ring_slots=0, ring_rows=0, store_entries=0)
    assert (h1["nbr"] == -1).all() and (h1["eid"] == -1).all() and not h1["nodes"].any() and not h1["memory"].any()
    # and the stream goes on from the emptied state as from a reset one
    e.observe_range(0, 100, B)
    torch.cuda.synchronize()
    e.check()
    assert int(e.ctl[CTL["ERR"]]) == 0 and int((e.loader.e_id >= 0).sum()) > 0


@pytest.mark.parametrize("N,ring,d", [(70, 4, 5), (70, 10, 16), (70, 32, 5), (257, 4, 16), (257, 10, 5), (257, 32, 16)])
def test_exact_over_shapes(N, ring, d):
    _exact_sequence("1hop_last", N, ring, d)


@pytest.mark.parametrize("form", [f for f in FORMS if f != "1hop_last"])
def test_exact_over_model_forms(form):
    _exact_sequence(form, 70, 10, 16)


def test_last_node_and_rows_that_straddle_nothing():
    """Node N - 1 as F and as a partner at N = 257, ring 10: row 256 is the only row of its wave's 6, and bit 0 of the
    bitmap's ninth word."""
    N = 257
    ev = make_events(5, 400, N, 5)
    ev["src"][-40:], ev["dst"][-40:] = N - 1, np.arange(40) * 6
    e = _engine(ev, N, ring=10)
    e.observe_range(0, 400, B)
    h0, h1, c = _check_forget(e, [N - 1])
    assert c["ring_rows"] >= 40 and h0["nodes"][N - 1, 1] > 0 and not h1["nodes"][N - 1].any()
    h0, h1, c = _check_forget(e, [0, N - 2, 254, 224])
    assert c["nodes"] == 4


@pytest.mark.parametrize("ring", [4, 10, 32])
def test_shuffled_t_stream_repairs_the_t_column(ring):
    """On a stream whose t is not ordered the ring's t column is ranked apart from e_id, so it is not the e_id column's
    times slot by slot: the forget re-ranks ev_t[e_id] of the survivors instead of dropping the same slots."""
    N = 70
    ev = _popular_stream(N, 5)
    ev["t"] = np.random.default_rng(4).permutation(ev["t"])
    e = _engine(ev, N, ring=ring)
    e.observe_range(0, 600, B)
    h0, h1, c = _check_forget(e, [11, 3, 40])
    assert c["ring_rows"] >= 60
    _, _, same_slots, _ = ring_forget(h0["nbr"], h0["eid"], h0["rt"], [11, 3, 40])
    assert not np.array_equal(_bits(same_slots), _bits(h1["rt"]))                 # (the two rules differ here)
    valid = h1["eid"] >= 0
    assert np.all(np.diff(h1["rt"], axis=1) <= 0)
    assert np.array_equal(np.sort(h1["rt"][valid]), np.sort(h1["t"][h1["eid"][valid]]))


@pytest.mark.parametrize("what", ["partner", "hub"])
def test_hub_runs_span_several_chunks(what):
    hub, N = 7, 70
    ev = hub_events(4, N, 16, hub=hub, B=200)
    e = _engine(ev, N, "1hop_mean", ring=10, max_batch=200)
    e.observe_range(0, 400, 200)
    torch.cuda.synchronize()
    assert e.model.store[4 * hub:4 * hub + 4].tolist()[1::2] == [150, 70]
    if what == "partner":
        ids = np.arange(10, N, 3)
        h0, h1, c = _check_forget(e, ids)
        assert 64 < h1["nodes"][hub, 1] < 150 and 0 < h1["nodes"][hub, 3] < 70
        assert h1["nodes"][hub, 0] == h0["nodes"][hub, 0] and h1["nodes"][hub, 2] == h0["nodes"][hub, 2]
    else:
        h0, h1, c = _check_forget(e, [hub])
        assert c["store_entries"] == 130 + 50 and not h1["nodes"][hub].any()      # less the 20 self loops, both ways
    e.observe_range(0, 200, 200)                                                  # the stream goes on
    torch.cuda.synchronize()
    e.check()


def test_forgotten_rows_equal_rows_added_by_grow_nodes():
    N = 70
    ev = _popular_stream(N, 16)
    a, twin = _engine(ev, N, ring=10), _engine(ev, N, ring=10)
    for e in (a, twin):
        e.observe_range(0, 600, B)
    F = [0, 11, 37, N - 1]
    a.forget_nodes(F)
    twin.grow_nodes(N + 1)
    ha, ht = _host(a), _host(twin)
    for k in STATE:
        if k != "arena":
            for v in F:
                assert np.array_equal(_bits(ha[k][v]), _bits(ht[k][N])), (k, v)
    assert int(a.loader._assoc.numel()) == N                                         # (nothing is resized)


@pytest.mark.parametrize("ring", [4, 10])
def test_compaction_retires_the_forgotten_rows(ring):
    N = 70
    ev = _popular_stream(N, 5)
    a, b = _engine(ev, N, ring=ring), _engine(ev, N, ring=ring)
    for e in (a, b):
        e.observe_range(0, 600, B)
    F = np.array([11, 3, 40, 41, 42])
    before = b.compact_events().numel()                       # what a compaction keeps without the forget
    b = _engine(ev, N, ring=ring)
    b.observe_range(0, 600, B)
    h0, h1, _ = _check_forget(b, F)
    kept_b = b.compact_events()
    h2 = _host(b)
    assert_same_deref(h1, h2)                                  # what the ring and the stores name is unchanged
    _same(h2, h1, ("memory", "last_update", "node_gen", "nbr", "rt"))
    out = a.forget_nodes(F, compact=True)
    ha = _host(a)
    assert torch.equal(out["kept"], kept_b) and set(out) == {"nodes", "ring_slots", "ring_rows", "store_entries", "kept"}
    _same(ha, h2, STATE + ("src", "dst", "t", "msg"))
    n = a.num_events
    assert 0 < n < before and not np.isin(ha["src"][:n], F).any() and not np.isin(ha["dst"][:n], F).any()
    a.check()


# ---------------------------------------------------------------------------------------------- semantics
def _sub(h, n):
    """The snapshot's first n nodes (deref compares what their ring rows and runs name)."""
    return dict(h, nbr=h["nbr"][:n], eid=h["eid"][:n], rt=h["rt"][:n], nodes=h["nodes"][:n])


@pytest.mark.parametrize("form", list(FORMS))
def test_component_twin(form):
    """Nodes [60, 70) interact among themselves only.  A observes everything, then forgets them and compacts; B is fed
    the same batches without their events and compacts: B runs only code that existed before forget_nodes."""
    N, d, nev = 70, 16, 600
    ev, comp = component_events(8, nev, d)
    one = {k: v[:1] for k, v in ev.items()}
    # (unflushed engines: a flush gives a never-seen node the row cell(0, 0), a forgotten or grown node has zeros)
    a, b = (_engine(one, N, form, ring=10, rows=1, flush=False) for _ in range(2))
    for e in (a, b):
        e.compact_events()                                      # (an empty table: the row the engine was built over goes)
        assert e.num_events == 0
    for s in range(0, nev, B):
        rows = np.arange(s, s + B)
        a.observe_events(*(ev[k][rows] for k in ("src", "dst", "t", "msg")), batch=B)
        keep = rows[~comp[rows]]
        b.observe_events(*(ev[k][keep] for k in ("src", "dst", "t", "msg")), batch=B)
    F = np.arange(60, 70)
    out = a.forget_nodes(F, compact=True)
    assert out["nodes"] == 10 and out["ring_slots"] == 0 and out["store_entries"] == 0    # nobody else named them
    b.compact_events()
    ha, hb = _host(a), _host(b)
    a.check()
    b.check()
    assert ha["n"] == hb["n"] > 0
    da, db = deref(_sub(ha, 60)), deref(_sub(hb, 60))
    for k in da:
        assert np.array_equal(da[k], db[k]), k
    assert (ha["nbr"][60:] == -1).all() and (hb["nbr"][60:] == -1).all()
    assert np.array_equal(ha["last_update"], hb["last_update"])
    err = float(np.abs(ha["memory"][:60] - hb["memory"][:60]).max())
    print(f"{form}: memory [0, 60) max err {err:.3e} (bound {MEM_TOL:.1e})")
    assert err <= MEM_TOL
    assert not ha["memory"][60:].any() and not hb["memory"][60:].any()
    _close(a.embed(torch.arange(60)), b.embed(torch.arange(60)), TOL)


def test_oracle_continuation():
    """Forget on both sides (the oracle through forget_ref), then three more observed batches, a flush and an eval
    batch at the tolerances of the step comparison."""
    r = Rig(aggr="last", N=70, B=50, d=16, D=32, nb=10, ring=10, max_neg=KN)
    eng, s = r.eng, r.s
    eng.flush()                             # (the oracle's first eval() is its train -> eval edge: it flushes there)
    for st in range(5):
        oracle_observe(r.ref, r.lref, s, r.ev_t, r.ev_msg, st * 50, (st + 1) * 50)
        eng.observe(st * 50, 50)
    seen = np.unique(np.concatenate([s.src[:250], s.dst[:250]]))
    F = np.concatenate([seen[::5], [int(s.dst[249]), int(s.src[249])]])
    h0 = _host(eng)
    want, counts = forget_ref(h0, F)
    got = eng.forget_nodes(F)
    assert {k: got[k] for k in counts} == counts and counts["ring_slots"] > 0 and counts["store_entries"] > 0
    _same(_host(eng), want, STATE)
    oracle_forget(r.ref, r.lref, F, s.t.astype(np.float32))

    def same_as_oracle():
        torch.cuda.synchronize()
        eng.check()
        err = float((eng.model.memory.memory.cpu() - r.ref.memory.memory).abs().max())
        print(f"memory max err {err:.3e} (bound {MEM_TOL:.1e})")
        assert err <= MEM_TOL
        assert torch.equal(eng.model.memory.last_update.cpu(), r.ref.memory.last_update)
        valid = r.lref.e_id >= 0
        assert np.array_equal(eng.loader.e_id.cpu().numpy(), r.lref.e_id)
        assert np.array_equal(eng.loader.neighbors.cpu().numpy()[valid], r.lref.neighbors[valid])
        assert np.array_equal(_bits(eng.loader.t.cpu().numpy()), _bits(r.lref.t))

    same_as_oracle()
    for st in range(5, 8):
        oracle_observe(r.ref, r.lref, s, r.ev_t, r.ev_msg, st * 50, (st + 1) * 50)
        eng.observe(st * 50, 50)
    same_as_oracle()
    r.ref.memory.training = True                                # (the oracle flushes on the train -> eval edge)
    negs = torch.from_numpy(np.random.default_rng(1).choice(s.dst_nodes, size=(50, KN)))
    r.flush_and_eval(8, negs)


def test_train_batch_after_a_forget_matches_a_twin_loaded_from_the_state():
    N, nev = 70, 400
    ev = _popular_stream(N, 16, nev)
    a = _engine(ev, N, ring=10, flush=False)
    a.observe_range(0, 300, B)
    a.forget_nodes([11, 3, 20])
    state = a.stream_state()
    c = _engine({k: v[:1] for k, v in ev.items()}, N, ring=10, flush=False, rows=1)
    c.load_stream_state(state)
    _same(_host(c), _host(a), STATE[:4] + STATE[5:] + ("src", "dst", "t", "msg"))
    neg = torch.from_numpy(np.random.default_rng(2).integers(0, N, B))
    for e in (a, c):
        e.train_batch(300, B, neg=neg, dropout=False)
    torch.cuda.synchronize()
    a.check()
    c.check()
    loss = float(a.model.grad_flat[-1])
    print(f"loss {loss:.6f}")
    assert np.isfinite(loss) and loss > 0 and torch.isfinite(a.model.memory.memory).all()
    _close(a.model.memory.memory, c.model.memory.memory, 1e-4)      # the train step's run-to-run bound
    assert torch.equal(a.model.memory.last_update, c.model.memory.last_update)
    assert torch.equal(a.loader.e_id, c.loader.e_id) and torch.equal(a.loader.neighbors, c.loader.neighbors)


@pytest.mark.parametrize("form", ["1hop_last", "2hop_mean"])
def test_embedding_table_restales_only_what_the_forget_touched(form):
    N = 257
    ev = make_events(6, 400, N - 2, 16)
    e = _engine(ev, N, form, ring=4, flush=False)
    e.enable_embedding_table()
    e.observe_range(0, 400, B)
    assert e.refresh_embeddings().numel() == N and e.refresh_embeddings().numel() == 0
    F = np.array([9, 100, 255])
    h0 = _host(e)
    e.forget_nodes(F)
    h1 = _host(e)
    rows = np.flatnonzero((h0["eid"] != h1["eid"]).any(1))                            # F's rows and the rewritten ones
    want = stale_ids(h1["nbr"], h1["eid"], np.concatenate([F, rows]), int(e.cfg.layers))
    got = e.refresh_embeddings().cpu().numpy()
    print(f"{form}: {got.size} of {N} rows re-embedded")
    assert np.array_equal(got, want) and F.size < got.size < N
    nodes = torch.arange(N)
    _close(e.embed_cached(nodes), e.embed(nodes), 2 * TOL)
    assert e.refresh_embeddings().numel() == 0
    _close(e.embed(torch.from_numpy(F)), e.embed(torch.tensor([N - 1] * 3)), TOL)    # as a never-seen node embeds


# ---------------------------------------------------------------------------------------------- lifecycle
def test_bindings_and_graphs_are_dropped_and_work_goes_on():
    N, nev = 70, 600
    ev = _popular_stream(N, 16, nev)
    e = _engine(ev, N, ring=10, flush=False)
    negs = torch.from_numpy(np.random.default_rng(9).integers(0, N, size=(100, KN)))
    e.bind_eval_resident(500, 600, B, negs)
    e.bind_resident(0, 500, B, dropout=False)
    e.begin_epoch()
    e.capture_resident()
    e.replay_resident()
    e.replay_resident()
    assert e._graphs is not None and e._prefetched and e.plan_table is not None and e._ev is not None
    # an empty list drops nothing and launches nothing
    ver = e.loader.version
    assert e.forget_nodes([]) == dict(nodes=0, ring_slots=0, ring_rows=0, store_entries=0)
    assert e._graphs is not None and e._prefetched and e.plan_table is not None and e.loader.version == ver
    h0, h1, c = _check_forget(e, [11, 2])
    assert c["ring_slots"] > 0
    assert e._graphs is None and not e._prefetched and e.plan_table is None and not hasattr(e, "_res_buf")
    assert e._ev is None and e._ev_graphs is None
    e.bind_resident(0, 500, B, dropout=False)
    e.resident_train_step()
    e.capture_resident()
    e.replay_resident()
    torch.cuda.synchronize()
    e.check()
    assert int(e.ctl[CTL["ERR"]]) == 0 and int(e.ctl[CTL["NB"]]) == 4
    assert torch.isfinite(e.model.memory.memory).all() and np.isfinite(e.loss_sum())
    e.flush()
    e.bind_eval_resident(500, 600, B, negs)
    e.capture_eval(group=0)
    e.replay_eval_n(2)
    torch.cuda.synchronize()
    e.check()
    assert int((e.eval_rr() > 0).sum()) == 100


def test_checkpoint_round_trips_a_forgotten_state():
    N = 70
    ev = _popular_stream(N, 5)
    a = _engine(ev, N, ring=4)
    a.observe_range(0, 500, B)
    a.forget_nodes([11, 0, N - 1])
    c = _engine({k: v[:1] for k, v in ev.items()}, N, ring=4, rows=1)
    c.load_stream_state(a.stream_state())
    ha, hc = _host(a), _host(c)
    _same(hc, ha, STATE[:4] + STATE[5:] + ("src", "dst", "t", "msg"))
    assert np.array_equal(hc["arena"][:2 * ha["n"]], ha["arena"][:2 * ha["n"]])
    rows = {k: v[500:600] for k, v in ev.items()}
    for e in (a, c):
        e.observe_events(rows["src"], rows["dst"], rows["t"], rows["msg"], batch=B)
    ha, hc = _host(a), _host(c)
    _same(hc, ha, STATE[:4] + STATE[5:])
    assert torch.equal(a.embed(torch.arange(N)), c.embed(torch.arange(N)))
    a.check()
    c.check()


@pytest.mark.parametrize("pool", ["all", None, "some"])
def test_drop_candidates(pool):
    N = 70
    ev = _popular_stream(N, 16)
    given = np.arange(5, 60) if pool == "some" else pool
    e = _engine(ev, N, ring=10, dst_nodes=given)
    e.observe_range(0, 600, B)
    F = [11, 6, 64, 6]
    src = torch.tensor([1, 2, 3])
    e2 = _engine(ev, N, ring=10, dst_nodes=given)
    e2.observe_range(0, 600, B)
    e2.forget_nodes(F)
    _, ids = e2.recommend(src, N)                               # without the flag a forgotten node stays a candidate
    assert np.isin([11, 6], ids.cpu().numpy()[0]).all() and (e2.dst_nodes is None) == (given is None)
    h0, h1, c = _check_forget(e, F, drop_candidates=True)
    base = np.arange(N) if given is None or isinstance(given, str) else given
    want = base[~np.isin(base, F)]
    assert e.dst_nodes.dtype == torch.long and np.array_equal(e.dst_nodes.cpu().numpy(), want)
    val, ids = e.recommend(src, N)
    ids = ids.cpu().numpy()
    assert not np.isin(ids, F).any()
    for r in ids:
        assert np.array_equal(np.sort(r[r >= 0]), want)         # every candidate left, and only those
    h2 = _host(e)                                               # (the embed of recommend advanced ctl GEN)
    with pytest.raises(ValueError, match="no candidate"):
        e.forget_nodes(np.arange(N), drop_candidates=True)
    _same(_host(e), h2, STATE + REST)
    assert np.array_equal(e.dst_nodes.cpu().numpy(), want)


@pytest.mark.parametrize("N,ring", [(70, 4), (257, 10), (70, 32)])
def test_loader_alone(N, ring):
    from tgnx.sampler import LastNeighborLoader
    ev = _popular_stream(N, 5)
    ld = LastNeighborLoader(N, ring, device=DEV)
    for s in range(0, 600, B):
        ld.insert(torch.from_numpy(ev["src"][s:s + B]), torch.from_numpy(ev["dst"][s:s + B]),
                  torch.from_numpy(ev["t"][s:s + B]))
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    for F in ([N - 1], [11, 0, 11], np.arange(N)):
        nbr, eid, rt, ver = g(ld.neighbors), g(ld.e_id), g(ld.t), ld.version
        wn, we, wt, counts = ring_forget(nbr, eid, rt, F)
        assert ld.forget(F) == counts and ld.version == ver + 1
        assert np.array_equal(g(ld.neighbors), wn) and np.array_equal(g(ld.e_id), we)
        assert np.array_equal(_bits(g(ld.t)), _bits(wt))
    assert ld.forget([]) == dict(nodes=0, ring_slots=0, ring_rows=0) and ld.version == ver + 1
    nbr = g(ld.neighbors)
    with pytest.raises(ValueError, match="node ids"):
        ld.forget([N])
    with pytest.raises(ValueError, match="node ids"):
        ld.forget([3, -1])
    assert np.array_equal(g(ld.neighbors), nbr) and ld.version == ver + 1
    ld.insert(torch.from_numpy(ev["src"][:B]), torch.from_numpy(ev["dst"][:B]), torch.from_numpy(ev["t"][:B]))
    assert int((ld.e_id >= 0).sum()) > 0                                              # the ring goes on


def test_loader_alone_equals_the_engine_on_a_time_ordered_stream():
    from tgnx.sampler import LastNeighborLoader
    N = 70
    ev = _popular_stream(N, 5)
    e = _engine(ev, N, ring=10)
    e.observe_range(0, 600, B)
    ld = LastNeighborLoader(N, 10, device=DEV)
    ld.neighbors.copy_(e.loader.neighbors)
    ld.e_id.copy_(e.loader.e_id)
    ld.t.copy_(e.loader.t)
    F = [11, 4, 33]
    out, alone = e.forget_nodes(F), ld.forget(F)
    assert alone == {k: out[k] for k in alone}
    assert torch.equal(ld.neighbors, e.loader.neighbors) and torch.equal(ld.e_id, e.loader.e_id)
    assert torch.equal(ld.t.view(torch.int32), e.loader.t.view(torch.int32))


def test_dropin_equals_the_engine_call():
    import pyg_epoch_utils
    N = 70
    ev = _popular_stream(N, 16)
    a, b = _engine(ev, N, ring=10), _engine(ev, N, ring=10)
    for e in (a, b):
        e.observe_range(0, 600, B)
    with pytest.raises(RuntimeError, match="no engine"):
        pyg_epoch_utils.forget(a.model, a.loader, [1])
    a.model._tgnx_engine, a._mode_train, a._bound = a, False, (0, 600, B)       # as train() / test() attach it
    F = [11, 3, 3]
    out = pyg_epoch_utils.forget(a.model, a.loader, F, compact=True, drop_candidates=True)
    want = b.forget_nodes(F, compact=True, drop_candidates=True)
    assert torch.equal(out.pop("kept"), want.pop("kept")) and out == want
    _same(_host(a), _host(b), STATE + ("src", "dst", "t", "msg", "n"))
    assert torch.equal(a.dst_nodes, b.dst_nodes) and a._bound is None and a.loader.cur_e_id == a.num_events


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_untouched():
    from tgnx import _lib
    N = 70
    ev = _popular_stream(N, 5)
    e = _engine(ev, N, ring=10)
    e.observe_range(0, 600, B)
    e.bind_eval_resident(500, 600, B, torch.zeros(100, KN, dtype=torch.long))
    before = _host(e)
    ver = e.loader.version
    for bad in ([N], [3, -1], [0, 1 << 40]):
        with pytest.raises(ValueError, match="node ids"):
            e.forget_nodes(bad)
    after = _host(e)
    _same(after, before, STATE + REST)
    assert e.loader.version == ver and e._ev is not None                     # no binding dropped either
    # a corrupted e_id (a copy of the ring tensor, as test_gpu_tgn_compact.py corrupts it) is counted, never followed
    good = e.loader.e_id
    slots = (e.loader.neighbors != -1).nonzero()[:2].tolist()
    bad = good.clone()
    bad[slots[0][0], slots[0][1]] = e.num_events
    bad[slots[1][0], slots[1][1]] = 1 << 40
    e.loader.e_id = bad
    try:
        before = _host(e)
        with pytest.raises(RuntimeError, match="nothing was changed"):
            e.forget_nodes([11])
        _same(_host(e), before, STATE + REST)
        ws, rec = e._forget_plan(torch.tensor([11], device=DEV))
        assert rec[4] == 2 and rec[5] == N and rec[6] == e.num_events
        # an apply on that record stores nothing (the record is checked on the device)
        rc = _lib.lib().tgnx_tgn_forget_apply(ctypes.byref(e.cfg), ctypes.byref(e._buffers(0)), e.num_events,
                                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), None, e._stream())
        assert rc == 0
        _same(_host(e), before, STATE + REST)
    finally:
        e.loader.e_id = good
    # a bad store run and a bad arena entry are counted too
    st = e.model.store
    v = int((st[:4 * N].view(N, 4)[:, 1] > 0).nonzero()[0])
    saved = st[4 * v:4 * v + 2].clone()
    ids = torch.tensor([11], device=DEV)
    st[4 * v] = 2 * e.num_events - 1
    st[4 * v + 1] = 2
    assert e._forget_plan(ids)[1][4] == 1
    st[4 * v + 1] = -3
    assert e._forget_plan(ids)[1][4] == 1
    st[4 * v:4 * v + 2] = saved
    off = int(saved[0])
    word = st[4 * N + off].clone()
    st[4 * N + off] = e.num_events
    assert e._forget_plan(ids)[1][4] == 1
    st[4 * N + off] = word
    ws, rec = e._forget_plan(ids)
    assert rec[4] == 0 and rec[0] == 1
    # an apply on a workspace no plan has written stores nothing
    blank = torch.zeros(ws.numel(), dtype=torch.uint8, device=DEV)
    rc = _lib.lib().tgnx_tgn_forget_apply(ctypes.byref(e.cfg), ctypes.byref(e._buffers(0)), e.num_events,
                                          ctypes.c_void_p(blank.data_ptr()), blank.numel(), None, e._stream())
    assert rc == 0
    _same(_host(e), after, STATE + REST)
    # one device only
    w = _engine(ev, N, ring=10, flush=False)
    w.world = 2
    with pytest.raises(ValueError, match="one device"):
        w.forget_nodes([1])
    w.world, w.dp = 1, True
    with pytest.raises(ValueError, match="one device"):
        w.forget_nodes([])
    e.check()
