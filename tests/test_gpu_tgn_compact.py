"""GPU tests of event-table compaction and stream-state checkpoints: tgnx_tgn_compact_plan / _apply,
TgnEngine.compact_events / stream_state / load_stream_state and the drop-in compact / save_stream / load_stream.

Setup as in test_gpu_tgn_observe.py: parameters from a RefTGN state dict, dropout 0, engines reset and flushed, moved
by observe / eval_batch only, so nothing is non-deterministic and comparisons are exact.  Shapes where the kernels
can go wrong: N = 64, msg_dim 16, D = 32, B = 50, ring 4 and 10, the 5,000-event wiki-shaped stream; 20,001 events
over 48 nodes at B = 200 (626 bitmap words: three scan workgroups of 256 words, the last word holding one row);
msg_dim 5 (rows not 16-byte aligned: the row gather's scalar path and its tail).

  live set          kept equals the numpy restatement of the definition (tests/compact_ref.py) exactly; n_live is at
                    most num_events / 4 and at least one row is live through a store only;
  dereferenced      per node the (neighbour, t, src / dst / t / msg row of e_id) tuples of the ring and the rows its
                    s and d runs name are bit-identical before and after; kept[e_id_new] == e_id_old; memory,
                    last_update, node_gen untouched; store size, capacities, ctl words;
  the stream goes on  twins A (compacts after 3,000 rows and again midway) and B (never): the same observe_events
                    chunks, then state, embed, recommend, an eval batch and a resident eval pass are equal, event ids
                    through the composed kept maps; all six forms of the observe test at ring 10, 1hop_last at ring 4;
  edges             a freshly reset engine, upto below num_events, a node that is the dst of 70 events of one batch,
                    src == dst, untouched nodes, a second compaction is the identity, a corrupted ring copy is counted
                    and refused with nothing changed, capacity / world / null-argument refusals;
  training goes on  train_batch on rows appended after a compaction against an uncompacted twin (memory 1e-4,
                    parameters 2e-5: the run-to-run bounds test_gpu_tgn_rccl.py / test_gpu_tgn_observe.py document for
                    the step's float atomics); a compaction between two prefetched resident steps;
  checkpoint        stream_state -> torch.save -> torch.load -> load_stream_state into an engine over a 1-row table,
                    then the same continuation is bit-equal; refusals; the drop-in wrappers."""
import ctypes
import io

import numpy as np
import pytest
import torch

from compact_ref import assert_same_deref, live_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, d, D, B, KN, NEV = 64, 16, 32, 50, 5, 5000
FORMS = {"1hop_last": dict(layers=1, aggr="last"), "1hop_mean": dict(layers=1, aggr="mean"),
         "2hop_last": dict(layers=2, aggr="last"), "2hop_mean": dict(layers=2, aggr="mean"),
         "rnn": dict(layers=1, aggr="last", updater="rnn"),
         "dyrep_emb": dict(layers=1, aggr="last", memory="dyrep", use_src_emb_in_msg=True)}
CTL = {"BATCH_START": 0, "CUR_EID": 1, "B": 2, "GEN": 3, "NB": 10, "ERR": 11}


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


_STREAMS, _SD = {}, {}


def _stream(nev=NEV, nodes=N, dim=d):
    from tgnx.synth import make_stream
    key = (nev, nodes, dim)
    if key not in _STREAMS:
        _STREAMS[key] = make_stream("tgbl-wiki", seed=5, num_events=nev, num_nodes=nodes, msg_dim=dim)
    return _STREAMS[key]


def _events(s, lo, hi):
    return dict(src=s.src[lo:hi], dst=s.dst[lo:hi], t=s.t[lo:hi].astype(np.float32), msg=s.msg[lo:hi])


def _sd(form, nodes=N, dim=d):
    from oracle.tgn_ref import RefTGN
    key = (form, nodes, dim)
    if key not in _SD:
        kw = dict(FORMS[form])
        kw.pop("memory", None)
        torch.manual_seed(0)
        _SD[key] = RefTGN(nodes, dim, hidden=D, dropout=0.0, **kw).state_dict()
    return _SD[key]


def _engine(s, form="1hop_last", ring=10, rows=NEV, max_batch=B, events=None, nodes=N, dim=d, flush=True, **ekw):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    model = TGNModel(nodes, rows, dim, D, DEV, ring=ring, max_batch=max_batch, max_neg=KN, dropout=0.0, **FORMS[form])
    model.load_reference_state(_sd(form, nodes, dim))
    eng = TgnEngine(model, LastNeighborLoader(nodes, ring, device=DEV),
                    events if events is not None else _events(s, 0, rows), TgnAdam(model, 1e-3),
                    dst_nodes=s.dst_nodes, seed=7, **ekw)
    eng.reset_state()
    if flush:
        eng.flush()
    return eng


def _host(eng):
    """Host copies of everything a compaction may touch (the table's valid rows; the whole store)."""
    torch.cuda.synchronize()
    m, ld, Nn = eng.model, eng.loader, eng.cfg.num_nodes
    st = m.store.cpu().numpy()
    g = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    return dict(n=eng.num_events, cap=eng.event_capacity, nbr=g(ld.neighbors), eid=g(ld.e_id), rt=g(ld.t),
                nodes=st[:4 * Nn].reshape(Nn, 4).copy(), arena=st[4 * Nn:].copy(), src=g(eng.src), dst=g(eng.dst),
                t=g(eng.t), msg=g(eng.msg), memory=g(m.memory.memory), last_update=g(m.memory.last_update),
                node_gen=g(m.node_gen), ctl=g(eng.ctl), flat=g(m.flat))


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _check_compaction(eng, upto=None, capacity=None):
    """compact_events against the restatement (live set) and the dereferenced state; returns (kept, before, after,
    ring-referenced set, store-referenced set)."""
    from tgnx import _lib
    h0 = _host(eng)
    want, ring, stores = live_rows(h0["nbr"], h0["eid"], h0["nodes"], h0["arena"], h0["n"], upto)
    kept = eng.compact_events(upto=upto, capacity=capacity)
    h1 = _host(eng)
    eng.check()
    k = kept.cpu().numpy()
    assert kept.dtype == torch.long and np.array_equal(k, want), (k.shape, want.shape)
    n_live = want.shape[0]
    assert eng.num_events == h1["n"] == n_live
    # the table rows, gathered in order
    for key in ("src", "dst", "t", "msg"):
        assert np.array_equal(_bits(h1[key]), _bits(h0[key][want])), key
    # what the ring and the stores name
    assert_same_deref(h0, h1)
    v = h0["nbr"] != -1
    assert np.array_equal(k[h1["eid"][v]], h0["eid"][v]) and np.array_equal(h1["eid"][~v], h0["eid"][~v])
    assert np.array_equal(h1["nodes"][:, [1, 3]], h0["nodes"][:, [1, 3]])
    n_arena = int(h0["nodes"][:, [1, 3]].sum())
    runs = h1["nodes"][:, [0, 2]][h1["nodes"][:, [1, 3]] > 0]
    assert n_arena <= 2 * n_live and (runs.size == 0 or int(runs.max()) < n_arena)      # repacked below 2 * n_live
    for key in ("memory", "last_update", "node_gen", "flat", "nbr", "rt"):
        assert np.array_equal(_bits(h1[key]), _bits(h0[key])), key
    # sizes, cursors, ctl
    cap = eng.event_capacity
    assert cap >= max(n_live, 1) and eng.cfg.num_events == cap == eng.model.num_events
    assert eng.model.store.numel() == int(_lib.lib().tgnx_tgn_store_words(ctypes.byref(eng.cfg))) == 4 * len(v) + 2 * cap
    assert all(x.shape[0] == cap for x in eng._tab) and eng.neg_train.shape[0] == cap
    assert int(eng.neg_train.abs().sum()) == 0 and (eng.out_ev is None or eng.out_ev.shape[0] == cap)
    assert eng.loader.cur_e_id == n_live
    for i in range(24):
        assert int(h1["ctl"][i]) == (n_live if i in (CTL["BATCH_START"], CTL["CUR_EID"]) else int(h0["ctl"][i])), i
    return kept, h0, h1, ring, stores


_OBSERVED = {}


def _observed(ring):
    """An engine over the whole 5,000-event stream, observed in batches of 50, then compacted once (checked)."""
    if ring not in _OBSERVED:
        s = _stream()
        e = _engine(s, ring=ring)
        e.observe_range(0, NEV, B)
        cap0, ver0 = e.event_capacity, e.loader.version
        out = _check_compaction(e)
        _OBSERVED[ring] = (e, cap0, ver0) + out
    return _OBSERVED[ring]


@pytest.mark.parametrize("ring", [4, 10])
def test_live_set_equals_the_restatement(ring):
    e, cap0, ver0, kept, h0, h1, in_ring, in_store = _observed(ring)
    n_live = kept.numel()
    print(f"ring {ring}: {n_live} live of {NEV}, {len(in_ring)} through the ring, {len(in_store - in_ring)} store only")
    assert 0 < n_live <= NEV // 4                        # not vacuous: most rows are dead
    assert len(in_store - in_ring) >= 1                  # and a row lives through a store alone
    assert torch.equal(kept, kept.sort().values) and kept.unique().numel() == n_live


@pytest.mark.parametrize("ring", [4, 10])
def test_dereferenced_state_is_unchanged(ring):
    e, cap0, ver0, kept, h0, h1, _, _ = _observed(ring)    # (_check_compaction compared the dereferenced state)
    n_live = kept.numel()
    assert n_live <= e.event_capacity < cap0 == NEV
    assert e.event_capacity == max(n_live + 1, n_live + n_live // 2)      # grown_capacity applied to n_live
    assert e.loader.version == ver0 + 1
    # a second compaction immediately after the first is the identity
    kept2, *_ = _check_compaction(e)
    assert torch.equal(kept2.cpu(), torch.arange(n_live))


def test_scan_over_three_workgroups_and_a_partial_word():
    """20,001 events over 48 nodes at B = 200; a 49th node occurs in rows 5 and 6 only, so that the first scan
    workgroup's 8,192 rows hold live rows too (the hot nodes' references are all recent)."""
    nev, nodes = 20001, 48
    s = _stream(nev, nodes)
    ev = _events(s, 0, nev)
    ev["src"], ev["dst"] = ev["src"].copy(), ev["dst"].copy()
    ev["dst"][5] = ev["src"][6] = nodes
    e = _engine(s, ring=10, rows=nev, max_batch=200, nodes=nodes + 1, events=ev)
    e.observe_range(0, nev, 200)
    assert (nev + 31) // 32 > 2 * 256 and nev % 32 == 1
    kept, h0, *_ = _check_compaction(e)
    k = kept.tolist()
    assert k[:2] == [5, 6] and k[-1] == nev - 1 and any(8192 <= x < 16384 for x in k)   # rows in every scan chunk
    assert kept.numel() <= nev // 4


def test_msg_dim_5_row_gather_tail():
    nev = 1000
    s = _stream(nev, N, 5)
    e = _engine(s, ring=4, rows=nev, dim=5)
    e.observe_range(0, nev, B)
    kept, *_ = _check_compaction(e)
    assert 0 < kept.numel() < nev
    # aligned and unaligned row starts both occur on either side of the gather
    old, new = kept.cpu().numpy(), np.arange(kept.numel())
    assert ((old % 4 == 0) & (new % 4 == 0)).any() and ((old % 4 != 0) | (new % 4 != 0)).any()


# ---------------------------------------------------------------------------------------------- the stream goes on
CHUNKS_1 = (50, 1, 137, 112, 700)       # observe_events calls before A's second compaction (per-call batching)
CHUNKS_2 = (450, 450)                   # and after it: rows [3000, 4900) in all
FIRST = 3000


def _negs(s):
    return torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(NEV, KN)))


def _same_through(a, b, gmap, train=False):
    """Twin a (compacted, own numbering; gmap[a's id] = b's id) against twin b."""
    ha, hb = _host(a), _host(b)
    assert ha["n"] == gmap.shape[0]
    ha2 = dict(ha)
    v = ha["nbr"] != -1
    assert np.array_equal(ha["nbr"], hb["nbr"]) and np.array_equal(_bits(ha["rt"]), _bits(hb["rt"]))
    assert np.array_equal(gmap[ha["eid"][v]], hb["eid"][v])
    assert np.array_equal(ha["last_update"], hb["last_update"])
    for key in ("src", "dst", "t", "msg"):
        assert np.array_equal(_bits(ha[key]), _bits(hb[key][gmap])), key
    assert_same_deref(ha2, hb)
    if not train:
        assert np.array_equal(_bits(ha["memory"]), _bits(hb["memory"]))
        assert np.array_equal(ha["node_gen"], hb["node_gen"])
        for name in ("GEN", "NB", "B", "ERR"):
            assert int(ha["ctl"][CTL[name]]) == int(hb["ctl"][CTL[name]]), name
        assert int(ha["ctl"][CTL["ERR"]]) == 0


def _run_stream_goes_on(form, ring):
    s = _stream()
    negs = _negs(s)
    a, b = (_engine(s, form, ring=ring, rows=FIRST) for _ in range(2))
    for e in (a, b):
        e.observe_range(0, FIRST, B)
    kept1 = a.compact_events().cpu().numpy()
    assert a.num_events == kept1.shape[0] < FIRST // 2
    gmap, lo = kept1, FIRST
    for chunks, compact in ((CHUNKS_1, True), (CHUNKS_2, False)):
        for n in chunks:
            ev = _events(s, lo, lo + n)
            sa, na = a.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"], batch=B)
            assert (sa, na) == (gmap.shape[0], n)
            assert b.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"], batch=B) == (lo, n)
            gmap = np.concatenate([gmap, np.arange(lo, lo + n)])
            lo += n
        if compact:
            kept2 = a.compact_events().cpu().numpy()
            gmap = gmap[kept2]                                       # the two kept maps compose
            assert a.num_events == gmap.shape[0] and np.all(np.diff(gmap) > 0)
    assert lo == 4900
    torch.cuda.synchronize()
    a.check()
    b.check()
    _same_through(a, b, gmap)
    nodes = torch.arange(N)
    assert torch.equal(a.embed(nodes), b.embed(nodes))
    src = torch.from_numpy(s.src[:7].copy())
    (va, ia), (vb, ib) = a.recommend(src, 5), b.recommend(src, 5)
    assert torch.equal(ia, ib) and torch.equal(va, vb)
    # one eval batch on the next 50 rows, each engine in its own numbering
    ev = _events(s, lo, NEV)
    sa, _ = a.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    sb, _ = b.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    assert sb == lo and sa == gmap.shape[0]
    gmap = np.concatenate([gmap, np.arange(lo, NEV)])
    outs = []
    for e, st in ((a, sa), (b, sb)):
        p, n, r = e.eval_batch(st, B, negs[lo:lo + B])
        outs.append((p.clone(), n.clone(), r.clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # a resident eval pass bound after the compaction, over the last 50 rows in batches of 25
    for e, st in ((a, sa), (b, sb)):
        e.bind_eval_resident(st + B, st + 2 * B, 25, negs[lo + B:lo + 2 * B])
        for _ in range(3):                                           # 2 batches and a step past the end
            e.eval_resident_step()
    torch.cuda.synchronize()
    a.check()
    b.check()
    assert torch.equal(a.eval_rr(), b.eval_rr()) and a.eval_mrr() == b.eval_mrr()
    _same_through(a, b, gmap)


@pytest.mark.parametrize("form", list(FORMS))
def test_the_stream_goes_on(form):
    _run_stream_goes_on(form, 10)


def test_the_stream_goes_on_ring_4():
    _run_stream_goes_on("1hop_last", 4)


# ---------------------------------------------------------------------------------------------- edge shapes
def test_compaction_of_a_freshly_reset_engine():
    s = _stream()
    a = _engine(s, ring=4, rows=100)
    b = _engine(s, ring=4, rows=100)
    kept, *_ = _check_compaction(a)
    assert kept.numel() == 0 and a.num_events == 0 and a.event_capacity == 1
    ev = _events(s, 0, 100)
    assert a.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"], batch=B) == (0, 100)
    b.observe_range(0, 100, B)
    torch.cuda.synchronize()
    a.check()
    _same_through(a, b, np.arange(100))


def test_upto_keeps_unobserved_rows_verbatim():
    s = _stream()
    a, b = (_engine(s, ring=4, rows=FIRST) for _ in range(2))
    for e in (a, b):
        e.observe_range(0, 2800, B)
    kept, h0, h1, *_ = _check_compaction(a, upto=2800)
    k = kept.cpu().numpy()
    n_live = k.shape[0]
    assert np.array_equal(k[-200:], np.arange(2800, FIRST)) and n_live < 1000
    a.observe_range(n_live - 200, n_live, B)
    b.observe_range(2800, FIRST, B)
    torch.cuda.synchronize()
    a.check()
    _same_through(a, b, k)
    with pytest.raises(ValueError, match="upto"):
        a.compact_events(upto=a.num_events + 1)
    with pytest.raises(ValueError, match="upto"):
        a.compact_events(upto=-1)


def test_a_run_longer_than_a_wave_self_loops_and_untouched_nodes():
    """Two batches at max_batch 128: a generic one, then one in which node `hub` is the destination of 70 events (its
    d run is longer than a wave and than the ring), with src == dst events; nodes 60-63 never occur."""
    s = _stream()
    src, dst = s.src[:256].copy() % 60, s.dst[:256].copy() % 60
    hub = 7
    src[128:256][src[128:256] == hub] = 8
    dst[128:256][dst[128:256] == hub] = 9
    dst[130:200] = hub
    dst[210] = src[210]
    dst[40] = src[40]
    ev = dict(src=src, dst=dst, t=s.t[:256].astype(np.float32), msg=s.msg[:256])
    e = _engine(s, "1hop_mean", ring=4, rows=256, max_batch=128, events=ev)
    e.observe(0, 128)
    e.observe(128, 128)
    torch.cuda.synchronize()
    e.check()
    assert int(e.model.store[4 * hub + 3]) == 70 and int((e.loader.neighbors[60:] != -1).sum()) == 0
    kept, h0, h1, ring, stores = _check_compaction(e)
    assert 128 <= kept.numel() < 256 and set(range(128, 256)) <= set(kept.tolist())
    kept2, *_ = _check_compaction(e)
    assert torch.equal(kept2.cpu(), torch.arange(kept.numel()))


def test_corrupted_ring_is_counted_and_refused():
    e, *_ = _observed(10)
    good = e.loader.e_id
    slots = (e.loader.neighbors != -1).nonzero()[:2].tolist()
    bad = good.clone()
    bad[slots[0][0], slots[0][1]] = e.num_events
    bad[slots[1][0], slots[1][1]] = -1
    e.loader.e_id = bad
    try:
        before = _host(e)
        ptrs = [x.data_ptr() for x in e._tab] + [e.model.store.data_ptr()]
        with pytest.raises(RuntimeError, match="nothing was changed"):
            e.compact_events()
        after = _host(e)
        for k in before:
            assert np.array_equal(_bits(np.asarray(before[k])), _bits(np.asarray(after[k]))), k
        assert ptrs == [x.data_ptr() for x in e._tab] + [e.model.store.data_ptr()]
        ws, n_live, n_arena, n_bad = e._compact_plan(e.num_events)       # the C plan call reports the count
        assert n_bad == 2 and n_live >= 0
    finally:
        e.loader.e_id = good
    # a bad store run is counted too, not walked
    st = e.model.store
    v = int((st[:4 * N].view(N, 4)[:, 1] > 0).nonzero()[0])
    saved = st[4 * v:4 * v + 2].clone()
    st[4 * v] = 2 * e.num_events - 1                    # s_off + s_cnt beyond the arena words of the valid rows
    st[4 * v + 1] = 2
    assert e._compact_plan(e.num_events)[3] == 1
    st[4 * v + 1] = -3
    assert e._compact_plan(e.num_events)[3] == 1
    st[4 * v:4 * v + 2] = saved
    assert e._compact_plan(e.num_events)[3] == 0
    torch.cuda.synchronize()
    e.check()


def test_refusals():
    from tgnx import _lib
    e, *_ = _observed(4)
    n = e.num_events
    before = _host(e)
    with pytest.raises(ValueError, match="capacity"):
        e.compact_events(capacity=n - 1)
    with pytest.raises(ValueError, match="capacity"):
        e.compact_events(capacity=0)
    after = _host(e)
    for k in before:
        assert np.array_equal(_bits(np.asarray(before[k])), _bits(np.asarray(after[k]))), k
    # an explicit capacity
    kept, *_ = _check_compaction(e, capacity=n + 7)
    assert e.event_capacity == n + 7 and torch.equal(kept.cpu(), torch.arange(n))
    # world = 2 engines
    s = _stream()
    w = _engine(s, ring=4, rows=100, flush=False, rank=0, world=2)
    for call in (lambda: w.compact_events(), lambda: w.stream_state(), lambda: w.load_stream_state(e.stream_state())):
        with pytest.raises(ValueError, match="one device"):
            call()
    # the C calls: null ctl / ws, and a workspace that is too small
    mid = _host(e)
    L = _lib.lib()
    nb = int(L.tgnx_tgn_compact_ws_bytes(ctypes.byref(e.cfg), n))
    assert nb > 0 and L.tgnx_tgn_compact_ws_bytes(None, n) == 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = [torch.zeros(8, dtype=torch.long, device=DEV) for _ in range(6)]
    P = ctypes.c_void_p

    def plan(b, w_ptr, w_bytes, cfg=None):
        return L.tgnx_tgn_compact_plan(ctypes.byref(e.cfg) if cfg is None else cfg, ctypes.byref(b), n, n, P(w_ptr),
                                       w_bytes, e._stream())

    def apply(b, w_ptr, w_bytes):
        return L.tgnx_tgn_compact_apply(ctypes.byref(e.cfg), ctypes.byref(b), n, 1, *(P(x.data_ptr()) for x in out), 8,
                                        P(w_ptr), w_bytes, e._stream())

    b0 = e._buffers(0)
    b0.ctl = 0
    for rc in (plan(b0, ws.data_ptr(), nb), apply(b0, ws.data_ptr(), nb), plan(e._buffers(0), 0, nb),
               apply(e._buffers(0), 0, nb), plan(e._buffers(0), ws.data_ptr(), nb - 256),
               apply(e._buffers(0), ws.data_ptr(), nb - 256)):
        assert rc == -1 and len(L.tgnx_last_error()) > 0                  # TGNX_EINVAL
    assert L.tgnx_tgn_compact_plan(None, ctypes.byref(e._buffers(0)), n, n, P(ws.data_ptr()), nb, e._stream()) == -1
    assert L.tgnx_tgn_compact_plan(ctypes.byref(e.cfg), ctypes.byref(e._buffers(0)), n, n + 1, P(ws.data_ptr()), nb,
                                   e._stream()) == -1
    torch.cuda.synchronize()
    assert int(ws.sum()) == 0 and all(int(x.abs().sum()) == 0 for x in out)
    # an apply on a workspace no plan has written stores nothing (the record is checked on the device)
    big = [torch.zeros(8 * 16, dtype=torch.float32, device=DEV) for _ in range(4)]
    store = torch.zeros(4 * N + 16, dtype=torch.long, device=DEV)
    keep = torch.zeros(8, dtype=torch.long, device=DEV)
    rc = L.tgnx_tgn_compact_apply(ctypes.byref(e.cfg), ctypes.byref(e._buffers(0)), n, 8,
                                  *(P(x.data_ptr()) for x in big), P(store.data_ptr()), P(keep.data_ptr()), 8,
                                  P(ws.data_ptr()), nb, e._stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(store.abs().sum()) == 0 and all(float(x.abs().sum()) == 0 for x in big)
    after = _host(e)
    for k in mid:
        assert np.array_equal(_bits(np.asarray(mid[k])), _bits(np.asarray(after[k]))), k
    e.check()


# ---------------------------------------------------------------------------------------------- training goes on
def test_training_goes_on_after_a_compaction():
    s = _stream()
    negs = _negs(s)
    a, b = (_engine(s, ring=10, rows=2000, flush=False) for _ in range(2))
    for e in (a, b):
        for st in (0, 1):
            e.train_batch(st * B, B, neg=negs[st * B:(st + 1) * B, 0], dropout=False)
        e.observe_range(2 * B, 2000, B)
    kept = a.compact_events().cpu().numpy()
    ev = _events(s, 2000, 2200)
    sa, _ = a.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    sb, _ = b.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    assert (sa, sb) == (kept.shape[0], 2000)
    for e, st0 in ((a, sa), (b, sb)):
        for j in range(2):
            e.train_batch(st0 + j * B, B, neg=negs[2000 + j * B:2000 + (j + 1) * B, 0], dropout=False)
    torch.cuda.synchronize()
    a.check()
    b.check()
    _same_through(a, b, np.concatenate([kept, np.arange(2000, 2200)]), train=True)
    _close(a.model.memory.memory, b.model.memory.memory, 1e-4)
    _close(a.model.flat, b.model.flat, 2e-5)


def test_compaction_between_two_prefetched_resident_steps():
    s = _stream()
    e = _engine(s, ring=10, rows=1000, flush=False)
    e.bind_eval_resident(900, 1000, B, _negs(s)[900:1000])
    e.bind_resident(0, 1000, B, dropout=False)
    e.begin_epoch()
    e.resident_train_step()
    e.resident_train_step()
    assert e._prefetched and e.plan_table is not None and hasattr(e, "_res_buf") and e._ev is not None
    kept = e.compact_events(upto=2 * B)               # rows [100, 1000) are not observed yet: kept verbatim
    n_live = kept.numel()
    assert torch.equal(kept[-900:].cpu(), torch.arange(100, 1000)) and n_live <= 1000
    assert not e._prefetched and e.plan_table is None and not hasattr(e, "_res_buf") and not hasattr(e, "_res")
    assert e._graphs is None and e._ev is None and e._ev_graphs is None
    e.bind_resident(n_live - 900, n_live, B, dropout=False)
    e.ctl[CTL["NB"]] = 0                              # the new binding's cursor: its first batch
    e.resident_train_step()
    e.resident_train_step()
    assert e._prefetched
    torch.cuda.synchronize()
    e.check()
    assert int(e.ctl[CTL["ERR"]]) == 0 and int(e.ctl[CTL["NB"]]) == 2
    assert int((e.loader.e_id >= n_live - 900).sum()) > 0          # the stepped rows are in the ring, renumbered
    assert int(e.loader.e_id.max()) < n_live - 900 + 2 * B


# ---------------------------------------------------------------------------------------------- checkpoint
def _continue(e, s, lo, negs):
    for n in (50, 137, 313):
        ev = _events(s, lo, lo + n)
        e.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"], batch=B)
        lo += n
    z = e.embed(torch.arange(N))
    val, ids = e.recommend(torch.from_numpy(s.src[:7].copy()), 5)
    ev = _events(s, lo, lo + B)
    st, _ = e.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    p, n_, r = e.eval_batch(st, B, negs[lo:lo + B])
    torch.cuda.synchronize()
    e.check()
    return [z, val, ids, p.clone(), n_.clone(), r.clone()]


def _assert_identical(a, b, skip_ctl=()):
    ha, hb = _host(a), _host(b)
    for k in ("n", "nbr", "eid", "rt", "src", "dst", "t", "msg", "memory", "last_update", "node_gen"):
        assert np.array_equal(_bits(np.asarray(ha[k])), _bits(np.asarray(hb[k]))), k
    for i in range(24):
        assert i in skip_ctl or int(ha["ctl"][i]) == int(hb["ctl"][i]), (i, ha["ctl"].tolist(), hb["ctl"].tolist())
    assert np.array_equal(ha["nodes"], hb["nodes"])
    assert np.array_equal(ha["arena"][:2 * ha["n"]], hb["arena"][:2 * ha["n"]])


@pytest.mark.parametrize("compacted", [True, False])
def test_checkpoint_round_trip(compacted, tmp_path):
    from tgnx.tgn import STREAM_STATE_KEYS
    s = _stream()
    negs = _negs(s)
    a = _engine(s, ring=10, rows=FIRST)
    a.observe_range(0, FIRST, B)
    if compacted:
        a.compact_events()
    state = a.stream_state()
    assert tuple(state) == STREAM_STATE_KEYS and state["format"] == 1 and state["num_events"] == a.num_events
    assert state["store_arena"].numel() == 2 * a.num_events and state["src"].numel() == a.num_events
    path = tmp_path / "stream.pt"
    torch.save(state, path)
    if compacted:
        assert path.stat().st_size < 200_000          # O(live rows): the uncompacted one is ~ 3000 x 100 B more
    loaded = torch.load(path, map_location="cpu")
    c = _engine(s, ring=10, rows=1)                   # a fresh engine over a 1-row table, the same parameters
    c.bind_eval_resident(0, 1, 1, negs[:1])
    c.load_stream_state(loaded)
    assert c._ev is None and c.num_events == a.num_events and c.loader.cur_e_id == a.num_events
    _assert_identical(a, c)
    for x, y in zip(_continue(a, s, FIRST, negs), _continue(c, s, FIRST, negs)):
        assert torch.equal(x, y)
    _assert_identical(a, c)


def test_checkpoint_refusals_write_nothing():
    s = _stream()
    e4, *_ = _observed(4)
    e10, *_ = _observed(10)
    before = _host(e10)
    with pytest.raises(ValueError, match="fingerprint"):
        e10.load_stream_state(e4.stream_state())                      # ring 4 into ring 10
    st = e10.stream_state()
    st["format"] = 2
    with pytest.raises(ValueError, match="format"):
        e10.load_stream_state(st)
    st = e10.stream_state()
    st["ctl"][CTL["ERR"]] = 4
    with pytest.raises(ValueError, match="error flags"):
        e10.load_stream_state(st)
    st = e10.stream_state()
    st["msg"] = st["msg"][:, :d - 1]
    with pytest.raises(ValueError, match="msg"):
        e10.load_stream_state(st)
    del st["e_id"]
    with pytest.raises(ValueError, match="missing"):
        e10.load_stream_state(st)
    after = _host(e10)
    for k in before:
        assert np.array_equal(_bits(np.asarray(before[k])), _bits(np.asarray(after[k]))), k


def test_dropin_wrappers_reach_the_same_state():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TGNModel
    assert pyg_epoch_utils.compact is tgn_epoch.compact and pyg_epoch_utils.save_stream is tgn_epoch.save_stream
    assert pyg_epoch_utils.load_stream is tgn_epoch.load_stream
    s = _stream()
    a, b = (_engine(s, ring=10, rows=2000) for _ in range(2))
    for e in (a, b):
        e.observe_range(0, 2000, B)
    with pytest.raises(RuntimeError, match="no engine"):
        pyg_epoch_utils.compact(a.model, a.loader)
    a.model._tgnx_engine, a._mode_train, a._bound = a, False, (0, 2000, B)      # as train() / test() attach it
    kept = pyg_epoch_utils.compact(a.model, a.loader)
    assert torch.equal(kept, b.compact_events()) and a.loader.cur_e_id == a.num_events and a._bound is None
    f = io.BytesIO()
    pyg_epoch_utils.save_stream(a.model, a.loader, f)
    f.seek(0)
    model = TGNModel(N, None, d, D, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(_sd("1hop_last"))
    nl = LastNeighborLoader(N, 10, device=DEV)
    n = pyg_epoch_utils.load_stream(model, nl, f, optimizer=TgnAdam(model, 1e-3), dst_nodes=s.dst_nodes)
    c = model._tgnx_engine
    assert n == a.num_events == c.num_events == nl.cur_e_id and c._mode_train is False
    _assert_identical(a, c)
    ev = _events(s, 2000, 2120)
    got = pyg_epoch_utils.observe(model, nl, ev["src"], ev["dst"], ev["t"], ev["msg"])
    assert got == b.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"])
    torch.cuda.synchronize()
    c.check()
    _assert_identical(b, c, skip_ctl=(9,))      # (SEED: the advance writes it from the engine's own seed, 0 here, 7 there)
