"""GPU tests of score-free stream ingestion: tgnx_tgn_observe_step, TgnEngine.observe / observe_range /
append_events / observe_events / reserve_events and the drop-in tgn_epoch.observe.

Setup: the small stream of test_gpu_tgn_query.py — 600 wiki-shaped events over 300 nodes (msg_dim 16, D = 32, ring
10, B = 50), parameters from a RefTGN state dict, dropout 0.  Engines are reset, flushed, then moved by eval batches
and observe only, so the parameters never move and nothing is non-deterministic.  Forms: layers in {1, 2} x aggr in
{last, mean}, the RNN updater, and DyRep with use_src_emb_in_msg (1 hop; the observe step then runs the eval forward
for the 2B endpoint roots).

  equals the eval step   twin engines, 3 eval batches each, then eval_batch with 5 negatives against observe on batches
             3-5: memory, last_update, store words, ring, node_gen and the ctl words GEN, NB, CUR_EID, BATCH_START, B,
             ERR (= 0) torch.equal.  Memory is bit-identical: the updater runs over the same sorted list with the same
             capacities on stored state (and, for DyRep, on embeddings whose rows depend on the endpoint's own ring row
             only);
  equals the oracle      the same batches through RefTGN.memory.update_state in eval mode and
             RefLastNeighborLoader.insert (DyRep: the embeddings passed as oracle.tgn_ref.eval_step passes them): memory
             within 2e-5 in the `_close` metric of test_gpu_tgn_query.py, last_update and ring exact;
  the stream goes on     both twins then run eval_batch on batch 6 with the same negatives: pos, neg, rr torch.equal,
             and embed() of the 120-node query set is equal;
  tiny graph  40 nodes, B = max_batch = 32, one negative (N < 2B: the observe step's root capacity is N): DyRep and
             2 hops, eval_batch against observe on batches 1-3, state torch.equal and the oracle's within 2e-5;
  append     an engine over the first 300 rows takes the other 300 in chunks of 50, 1, 137, 112 through
             observe_events(batch=50) — batching is per call, so the batches are [300,350) [350,351) [351,401) [401,451)
             [451,488) [488,538) [538,588) [588,600), which differ from a batching of [300, 600) by 50: the twin over
             all 600 rows runs observe_range per chunk to observe the same batches.  Capacity goes 300 -> 450 -> 675
             (two reallocations); all state, num_events, recommend() and a resident eval pass bound afterwards agree;
  shapes     a node that is an endpoint of 15 events of one batch (ring 10), src == dst, B = 1, B = max_batch,
             B = 0 (nothing changes), B > max_batch / rows beyond num_events (ValueError), append_events with an id of
             -1 or N (ValueError, nothing changes), the C call with a null ctl / ws (TGNX_EINVAL);
  training goes on       train_batch 0-1, then eval_batch(2) against observe(2), then train_batch(3): ring, stores,
             last_update exact, memory within 1e-4 and parameters within 2e-5 (the run-to-run bounds
             test_gpu_tgn_rccl.py documents for the step's float atomics); an observe between two prefetched resident
             steps clears _prefetched and the next step prepares its batch again;
  drop-in    pyg_epoch_utils.observe after train() flushes once and equals a hand-flushed twin's observe_events."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, d, D, B, KN, NEV = 300, 16, 32, 50, 5, 600
TOL = 2e-5
FORMS = {"1hop_last": dict(layers=1, aggr="last"), "1hop_mean": dict(layers=1, aggr="mean"),
         "2hop_last": dict(layers=2, aggr="last"), "2hop_mean": dict(layers=2, aggr="mean"),
         "rnn": dict(layers=1, aggr="last", updater="rnn"),
         "dyrep_emb": dict(layers=1, aggr="last", memory="dyrep", use_src_emb_in_msg=True)}
CTL = {"BATCH_START": 0, "CUR_EID": 1, "B": 2, "GEN": 3, "NB": 10, "ERR": 11}
STATE = ("memory", "last_update", "store", "node_gen", "neighbors", "e_id", "t")


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _stream():
    from tgnx.synth import make_stream
    return make_stream("tgbl-wiki", seed=5, num_events=NEV, num_nodes=N, msg_dim=d)


def _events(s, lo=0, hi=NEV):
    return dict(src=s.src[lo:hi], dst=s.dst[lo:hi], t=s.t[lo:hi].astype(np.float32), msg=s.msg[lo:hi])


def _engine(s, sd, form, rows=NEV, max_batch=B, events=None):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    kw = dict(FORMS[form]) if isinstance(form, str) else dict(form)
    model = TGNModel(N, rows, d, D, DEV, ring=10, max_batch=max_batch, max_neg=KN, dropout=0.0, **kw)
    model.load_reference_state(sd)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=DEV), events if events is not None else _events(s, 0, rows),
                    TgnAdam(model, 1e-3), dst_nodes=s.dst_nodes, seed=7)
    eng.reset_state()
    return eng


def _ref(form):
    from oracle.tgn_ref import RefTGN
    kw = dict(FORMS[form])
    kw.pop("memory", None)
    torch.manual_seed(0)
    return RefTGN(N, d, hidden=D, dropout=0.0, **kw)


def _negs(s):
    return torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(8 * B, KN)))


def _eval(eng, negs, first, count, batch=B):
    out = []
    for st in range(first, first + count):
        p, n, r = eng.eval_batch(st * batch, batch, negs[st * batch:(st + 1) * batch])
        out.append((p.clone(), n.clone(), r.clone()))
    torch.cuda.synchronize()
    eng.check()
    return out


def _state(eng):
    m, ld = eng.model, eng.loader
    return dict(memory=m.memory.memory, last_update=m.memory.last_update, store=m.store, node_gen=m.node_gen,
                neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t, flat=m.flat, ctl=eng.ctl)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _assert_same_state(a, b, keys=STATE, ctl=True, store_words=None):
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in keys:
        x, y = sa[k], sb[k]
        if k == "store" and store_words is not None:      # (engines of different table capacity: the common words)
            x, y = x[:store_words], y[:store_words]
        assert torch.equal(_bits(x), _bits(y)), k
    if ctl:
        for name, i in CTL.items():
            assert int(sa["ctl"][i]) == int(sb["ctl"][i]), (name, sa["ctl"].tolist(), sb["ctl"].tolist())
        assert int(sa["ctl"][CTL["ERR"]]) == 0


def _query_nodes(s, events):
    seen = np.concatenate([s.src[:events], s.dst[:events]])
    hub = int(np.bincount(seen, minlength=N).argmax())
    empty = int(np.setdiff1d(np.arange(N), seen)[0])
    rnd = np.random.default_rng(3).integers(0, N, 114)
    return np.concatenate([[hub, empty, hub], rnd, [empty, int(rnd[0]), int(rnd[1])]]).astype(np.int64)


_TWINS = {}


def _twins(form):
    """(stream, negatives, A, B, B's state after batch 5) per form, built once: 3 eval batches on both, then A
    eval_batch / B observe on batches 3-5.  `test_the_stream_goes_on` moves both the same way."""
    if form not in _TWINS:
        s = _stream()
        sd = _ref(form).state_dict()
        negs = _negs(s)
        a, b = (_engine(s, sd, form) for _ in range(2))
        for e in (a, b):
            e.flush()
            _eval(e, negs, 0, 3)
        _eval(a, negs, 3, 3)
        for st in range(3, 6):
            b.observe(st * B, B)
        torch.cuda.synchronize()
        b.check()
        snap = {k: v.clone() for k, v in _state(b).items()}          # B after batch 5, whatever runs later
        _TWINS[form] = (s, negs, a, b, snap)
    return _TWINS[form]


@pytest.mark.parametrize("form", list(FORMS))
def test_observe_equals_the_eval_step(form):
    s, negs, a, b, snap = _twins(form)
    _assert_same_state(a, b)
    assert int(snap["ctl"][CTL["B"]]) == B and int(snap["ctl"][CTL["BATCH_START"]]) == 5 * B
    assert torch.equal(_bits(_state(a)["flat"]), _bits(_state(b)["flat"]))          # parameters untouched


@pytest.mark.parametrize("form", list(FORMS))
def test_observe_equals_the_oracle_update_state(form):
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import _emb_args, eval_step, sample_hops
    s, negs, _, _, sb = _twins(form)
    ref = _ref(form)
    lref = RefLastNeighborLoader(N, 10)
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    src, dst = torch.from_numpy(s.src), torch.from_numpy(s.dst)
    for st in range(3):
        sl = slice(st * B, (st + 1) * B)
        eval_step(ref, lref, ev_t, ev_msg, src[sl], dst[sl], negs[sl], ev_t[sl], ev_msg[sl])
    ref.eval()
    with torch.no_grad():
        for st in range(3, 6):
            sl = slice(st * B, (st + 1) * B)
            emb = ()
            if ref.memory.use_src_emb_in_msg or ref.memory.use_dst_emb_in_msg:
                # the batch's embeddings over the sampled set of src ∪ dst, as eval_step passes them
                n_id, ei, e_id = sample_hops(ref, lref, torch.cat([src[sl], dst[sl]]).unique().numpy())
                assoc = torch.zeros(N, dtype=torch.long)
                assoc[n_id] = torch.arange(n_id.size(0))
                z, lu = ref.memory(n_id)
                z = ref.gnn(z, lu, ei, ev_t[e_id], ev_msg[e_id])
                emb = _emb_args(ref, z, assoc)
            ref.memory.update_state(src[sl], dst[sl], ev_t[sl], ev_msg[sl], *emb)
            lref.insert(s.src[sl], s.dst[sl], s.t[sl].astype(np.float32))
    _close(sb["memory"], ref.memory.memory, TOL)
    assert torch.equal(sb["last_update"].cpu(), ref.memory.last_update)
    assert np.array_equal(sb["neighbors"].cpu().numpy(), lref.neighbors)
    assert np.array_equal(sb["e_id"].cpu().numpy(), lref.e_id)
    assert np.array_equal(sb["t"].cpu().numpy(), lref.t.astype(np.float32))


@pytest.mark.parametrize("form", list(FORMS))
def test_the_stream_goes_on(form):
    s, negs, a, b, _ = _twins(form)
    (pa, na, ra), = _eval(a, negs, 6, 1)
    (pb, nb, rb), = _eval(b, negs, 6, 1)
    assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(ra, rb)
    nodes = _query_nodes(s, 7 * B)
    assert torch.equal(a.embed(nodes), b.embed(nodes))
    _assert_same_state(a, b, ctl=False)


@pytest.mark.parametrize("form", ["dyrep_emb", "2hop_last"])
def test_observe_on_a_graph_smaller_than_two_batches(form):
    """N = 40 < 2B = 64 (max_batch = B = 32, one negative, 4 batches of the 128-event stream): the observe step's root
    capacity is min(N, 2B) = N, as the eval step's min(N, B (2 + Kn)) is.  Batch 0 by eval_batch on both twins, then
    batches 1-3 by eval_batch against observe: state torch.equal; and against the oracle's update_state within TOL."""
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN, _emb_args, eval_step, sample_hops
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    n, b, nev = 40, 32, 128
    s = make_stream("tgbl-wiki", seed=5, num_events=nev, num_nodes=n, msg_dim=d)
    kw = dict(FORMS[form])
    okw = {k: v for k, v in kw.items() if k != "memory"}
    torch.manual_seed(0)
    ref = RefTGN(n, d, hidden=D, dropout=0.0, **okw)
    negs = torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(nev, 1)))
    twins = []
    for _ in range(2):
        model = TGNModel(n, nev, d, D, DEV, ring=10, max_batch=b, max_neg=1, dropout=0.0, **kw)
        model.load_reference_state(ref.state_dict())
        e = TgnEngine(model, LastNeighborLoader(n, 10, device=DEV), _events(s, 0, nev), TgnAdam(model, 1e-3),
                      dst_nodes=s.dst_nodes, seed=7)
        e.reset_state()
        e.flush()
        _eval(e, negs, 0, 1, batch=b)
        twins.append(e)
    x, y = twins
    assert n < 2 * b and int(y.cfg.max_batch) == b
    _eval(x, negs, 1, 3, batch=b)
    for st in range(1, 4):
        y.observe(st * b, b)
    torch.cuda.synchronize()
    y.check()
    _assert_same_state(x, y)
    lref = RefLastNeighborLoader(n, 10)
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    src, dst = torch.from_numpy(s.src), torch.from_numpy(s.dst)
    eval_step(ref, lref, ev_t, ev_msg, src[:b], dst[:b], negs[:b], ev_t[:b], ev_msg[:b])
    ref.eval()
    with torch.no_grad():
        for st in range(1, 4):
            sl = slice(st * b, (st + 1) * b)
            emb = ()
            if ref.memory.use_src_emb_in_msg or ref.memory.use_dst_emb_in_msg:
                n_id, ei, e_id = sample_hops(ref, lref, torch.cat([src[sl], dst[sl]]).unique().numpy())
                assoc = torch.zeros(n, dtype=torch.long)
                assoc[n_id] = torch.arange(n_id.size(0))
                z, lu = ref.memory(n_id)
                z = ref.gnn(z, lu, ei, ev_t[e_id], ev_msg[e_id])
                emb = _emb_args(ref, z, assoc)
            ref.memory.update_state(src[sl], dst[sl], ev_t[sl], ev_msg[sl], *emb)
            lref.insert(s.src[sl], s.dst[sl], s.t[sl].astype(np.float32))
    sy = _state(y)
    _close(sy["memory"], ref.memory.memory, TOL)
    assert torch.equal(sy["last_update"].cpu(), ref.memory.last_update)
    assert np.array_equal(sy["neighbors"].cpu().numpy(), lref.neighbors)
    assert np.array_equal(sy["e_id"].cpu().numpy(), lref.e_id)
    assert np.array_equal(sy["t"].cpu().numpy(), lref.t.astype(np.float32))


CHUNKS = (50, 1, 137, 112)


@pytest.mark.parametrize("form", ["1hop_last", "2hop_mean"])
def test_append_and_observe_equal_a_table_bound_whole(form):
    s = _stream()
    sd = _ref(form).state_dict()
    c = _engine(s, sd, form, rows=300)
    w = _engine(s, sd, form)
    assert c.num_events == c.event_capacity == c.cfg.num_events == 300 and w.num_events == NEV
    for e in (c, w):
        e.flush()
        e.observe_range(0, 300, B)
    caps, ptrs, lo = [c.event_capacity], [tuple(x.data_ptr() for x in (c.src, c.dst, c.t, c.msg))], 300
    for n in CHUNKS:
        ev = _events(s, lo, lo + n)
        got = c.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"], batch=B)
        assert got == (lo, n)
        w.observe_range(lo, lo + n, B)                  # the same per-call batches
        lo += n
        caps.append(c.event_capacity)
        ptrs.append(tuple(x.data_ptr() for x in (c.src, c.dst, c.t, c.msg)))
    assert caps == [300, 450, 450, 675, 675], caps
    moved = [i for i in range(1, len(ptrs)) if all(p != q for p, q in zip(ptrs[i], ptrs[i - 1]))]
    assert moved == [1, 3], (moved, ptrs)               # the four tensors were reallocated twice
    assert c.num_events == w.num_events == NEV and c.cfg.num_events == 675 and c.neg_train.numel() == 675
    for k in ("src", "dst", "t", "msg"):
        assert torch.equal(getattr(c, k), getattr(w, k)), k
    torch.cuda.synchronize()
    c.check()
    w.check()
    _assert_same_state(c, w, store_words=4 * N + 2 * NEV)
    src = torch.from_numpy(s.src[:7].copy())
    (vc, ic), (vw, iw) = c.recommend(src, 5), w.recommend(src, 5)
    assert torch.equal(ic, iw) and torch.equal(vc, vw)
    # a resident eval pass bound after the appends, over appended rows
    negs = _negs(s)[:150]
    for e in (c, w):
        e.bind_eval_resident(450, NEV, B, negs)
        for _ in range(4):                              # 3 batches and a step past the end
            e.eval_resident_step()
    torch.cuda.synchronize()
    c.check()
    assert torch.equal(c.eval_rr(), w.eval_rr()) and c.eval_mrr() == w.eval_mrr()
    _assert_same_state(c, w, ctl=False, store_words=4 * N + 2 * NEV)


def _odd_stream():
    """The stream with batch 3 rewritten: one node the source of 9 and the destination of 6 of its events (15 > the
    ring's 10), and one event with src == dst."""
    s = _stream()
    src, dst = s.src.copy(), s.dst.copy()
    hub = int(src[150])
    src[150:159] = hub
    dst[160:166] = hub
    dst[170] = src[170]
    return s, dict(src=src, dst=dst, t=s.t.astype(np.float32), msg=s.msg), hub


def test_shapes_where_it_can_go_wrong():
    s, ev, hub = _odd_stream()
    sd = _ref("1hop_mean").state_dict()
    negs = _negs(s)
    a, b = (_engine(s, sd, "1hop_mean", events=ev) for _ in range(2))
    for e in (a, b):
        e.flush()
        _eval(e, negs, 0, 3)
    steps = [(150, 50), (200, 1), (201, 50), (251, 1)]  # the hub / self-loop batch, B = 1, B = max_batch, B = 1
    for start, n in steps:
        a.eval_batch(start, n, negs[start:start + n])
        b.observe(start, n)
        _assert_same_state(a, b)
    b.check()
    both = np.concatenate([ev["src"][150:200], ev["dst"][150:200]])
    assert int((both == hub).sum()) >= 15 and int((b.loader.e_id[hub] >= 150).sum()) == 10
    # B = 0: nothing moves (GEN and NB advance with the batch descriptor, as for any advance)
    before = {k: v.clone() for k, v in _state(b).items()}
    b.observe(252, 0)
    b.observe(NEV, 0)
    torch.cuda.synchronize()
    b.check()
    for k in STATE + ("flat",):
        assert torch.equal(_bits(_state(b)[k]), _bits(before[k])), k
    # and the next batch is still the eval step's (B's generation is two advances ahead, and so are its stamps)
    a.eval_batch(252, 50, negs[252:302])
    b.observe(252, 50)
    _assert_same_state(a, b, keys=tuple(k for k in STATE if k != "node_gen"), ctl=False)
    sa, sb = _state(a), _state(b)
    assert int(sb["ctl"][CTL["GEN"]]) == int(sa["ctl"][CTL["GEN"]]) + 2
    assert torch.equal(sb["node_gen"] == sb["ctl"][CTL["GEN"]], sa["node_gen"] == sa["ctl"][CTL["GEN"]])
    # refused before any launch
    gen = int(b.ctl[CTL["GEN"]])
    for start, n in ((0, B + 1), (NEV - B + 1, B), (NEV, 1), (-1, 5), (0, -1)):
        with pytest.raises(ValueError):
            b.observe(start, n)
    with pytest.raises(ValueError):
        b.observe_range(0, NEV + 1, B)
    with pytest.raises(ValueError):
        b.observe_range(0, NEV, B + 1)
    assert int(b.ctl[CTL["GEN"]]) == gen


def test_append_events_validates_before_anything_is_written():
    s = _stream()
    sd = _ref("1hop_last").state_dict()
    e = _engine(s, sd, "1hop_last", rows=300)
    e.flush()
    e.observe_range(0, 300, B)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(e).items()}
    table = [x.clone() for x in (e.src, e.dst, e.t, e.msg)]
    ptr = e.src.data_ptr()
    ev = _events(s, 300, 400)
    for bad_id, side in ((-1, "src"), (N, "src"), (-1, "dst"), (N, "dst")):
        rows = {k: np.array(v, copy=True) for k, v in ev.items()}
        rows[side][37] = bad_id
        with pytest.raises(ValueError, match="node ids"):
            e.append_events(rows["src"], rows["dst"], rows["t"], rows["msg"])
        with pytest.raises(ValueError, match="node ids"):
            e.observe_events(rows["src"], rows["dst"], rows["t"], rows["msg"], batch=B)
    with pytest.raises(ValueError, match="msg"):
        e.append_events(ev["src"], ev["dst"], ev["t"], ev["msg"][:, :d - 1])
    with pytest.raises(ValueError, match="one length"):
        e.append_events(ev["src"], ev["dst"][:99], ev["t"], ev["msg"])
    torch.cuda.synchronize()
    assert e.num_events == 300 and e.event_capacity == 300 and e.src.data_ptr() == ptr
    for x, y in zip((e.src, e.dst, e.t, e.msg), table):
        assert torch.equal(x, y)
    for k in STATE + ("flat", "ctl"):
        assert torch.equal(_bits(_state(e)[k]), _bits(before[k])), k
    # unvalidated: no host read, the ids are clamped into [0, N) instead of reaching a kernel as an index
    rows = {k: np.array(v, copy=True) for k, v in ev.items()}
    rows["src"][3], rows["dst"][4] = -7, N + 5
    assert e.append_events(rows["src"], rows["dst"], rows["t"], rows["msg"], validate=False) == (300, 100)
    assert int(e.src[303]) == 0 and int(e.dst[304]) == N - 1 and e.num_events == 400
    assert e.append_events([], [], [], np.zeros((0, d), np.float32)) == (400, 0)
    # reserve_events: capacity ahead of time, rows and state kept
    e.reserve_events(1000)
    assert e.event_capacity == 1000 and e.cfg.num_events == 1000 and e.num_events == 400
    assert torch.equal(e.src[:300], table[0]) and torch.equal(e.msg[:300], table[3])
    e.reserve_events(10)
    assert e.event_capacity == 1000
    e.observe_range(300, 400, B)
    torch.cuda.synchronize()
    e.check()


def test_c_call_refuses_null_buffers():
    from tgnx import _lib
    s = _stream()
    e = _engine(s, _ref("1hop_last").state_dict(), "1hop_last")
    e.advance(0, B, False)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(e).items()}
    L = _lib.lib()
    for field in ("ctl", "ws"):
        b = e._buffers(0)
        setattr(b, field, 0)
        rc = L.tgnx_tgn_observe_step(ctypes.byref(e.cfg), ctypes.byref(b), e._stream())
        assert rc == -1 and len(L.tgnx_last_error()) > 0                  # TGNX_EINVAL
    assert L.tgnx_tgn_observe_step(None, ctypes.byref(e._buffers(0)), e._stream()) == -1
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(_bits(_state(e)[k]), _bits(before[k])), k
    # neg / out_pos / out_neg / mrr are not read: the call runs with all four null
    b = e._buffers(0)
    b.neg = b.out_pos = b.out_neg = b.mrr = 0
    assert L.tgnx_tgn_observe_step(ctypes.byref(e.cfg), ctypes.byref(b), e._stream()) == 0
    torch.cuda.synchronize()
    e.check()
    assert int((e.loader.e_id >= 0).sum()) > 0


def test_training_goes_on():
    s = _stream()
    sd = _ref("1hop_last").state_dict()
    negs = _negs(s)
    a, b = (_engine(s, sd, "1hop_last") for _ in range(2))
    for e in (a, b):
        for st in (0, 1):
            e.train_batch(st * B, B, neg=negs[st * B:(st + 1) * B, 0], dropout=False)
    a.eval_batch(2 * B, B, negs[2 * B:3 * B])
    b.observe(2 * B, B)
    for e in (a, b):
        e.train_batch(3 * B, B, neg=negs[3 * B:4 * B, 0], dropout=False)
    torch.cuda.synchronize()
    a.check()
    b.check()
    _assert_same_state(a, b, keys=("neighbors", "e_id", "t", "store", "last_update"), ctl=False)
    _close(_state(b)["memory"], _state(a)["memory"], 1e-4)
    _close(_state(b)["flat"], _state(a)["flat"], 2e-5)


def test_observe_between_two_prefetched_steps():
    """The prefetch trap: a parity-set, gather-ahead step has already marked, scanned and gathered the NEXT batch in
    the workspace observe reuses; observe must make the next step prepare its batch again.  The twin runs the same
    calls with steps that prepare their own batch every time (pipeline off, gather-ahead off), so nothing of it is
    ever prepared ahead.  (Not compared with eval_batch here: a prefetched step stamps the next batch's endpoints with
    the generation the following advance hands out, so an eval batch in this place also updates those of its
    candidates that are among them; observe marks its own endpoints only.)"""
    s = _stream()
    sd = _ref("1hop_last").state_dict()
    a, b = (_engine(s, sd, "1hop_last") for _ in range(2))
    a.pipeline = a.gather_ahead = False
    for e in (a, b):
        e.bind_resident(0, NEV, B, dropout=False)
        e.begin_epoch()
        e.resident_train_step()
        e.resident_train_step()
    assert b.gather_ahead and b.parity_sets and b._prefetched and not a._prefetched
    for e in (a, b):
        e.observe(10 * B, B)
        assert not e._prefetched
        e.resident_train_step()
    assert b._prefetched
    torch.cuda.synchronize()
    a.check()
    b.check()
    assert int((b.loader.e_id >= 10 * B).sum()) > 0                       # the observed rows are in the ring
    _assert_same_state(a, b, keys=("neighbors", "e_id", "t", "store", "last_update"), ctl=False)
    _close(_state(b)["memory"], _state(a)["memory"], 1e-4)
    _close(_state(b)["flat"], _state(a)["flat"], 2e-5)
    assert int(a.ctl[CTL["NB"]]) == int(b.ctl[CTL["NB"]]) == 4


def test_dropin_observe_flushes_once_and_equals_a_hand_flushed_twin():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.data import SplitLoader, TemporalData
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TGNModel
    s = _stream()
    sd = _ref("1hop_last").state_dict()
    data = TemporalData(src=torch.from_numpy(s.src), dst=torch.from_numpy(s.dst), t=torch.from_numpy(s.t),
                        msg=torch.from_numpy(s.msg))
    loader = SplitLoader(data, 0, 4 * B, B, np.zeros(4 * B, dtype=np.int64))
    model = TGNModel(N, NEV, d, D, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(sd)
    nl = LastNeighborLoader(N, 10, device=DEV)
    ev = _events(s, 4 * B, 4 * B + 120)
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.observe(model, nl, ev["src"], ev["dst"], ev["t"], ev["msg"])
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train and eng.num_events == NEV
    stores = lambda m: int(m.store[:4 * N].view(N, 4)[:, [1, 3]].sum())  # noqa: E731
    assert stores(model) > 0
    twin = _engine(s, sd, "1hop_last")
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(twin).items():
            v.copy_(_state(eng)[k])
    twin.flush()
    want = twin.observe_events(ev["src"], ev["dst"], ev["t"], ev["msg"])          # batches of max_batch: 50, 50, 20
    got = pyg_epoch_utils.observe(model, nl, ev["src"], ev["dst"], ev["t"], ev["msg"])
    assert got == want == (NEV, 120) and nl.cur_e_id == NEV + 120
    assert not eng._mode_train and eng.num_events == twin.num_events == NEV + 120
    assert eng.event_capacity == NEV + NEV // 2 and eng.out_ev.shape[0] == eng.cfg.num_events == eng.event_capacity
    torch.cuda.synchronize()
    eng.check()
    _assert_same_state(eng, twin, ctl=False)
    # in eval mode already: a second call does not flush again (a flush would clear the stores observe just wrote)
    n_stored = stores(model)
    assert n_stored > 0
    e2 = _events(s, 500, 530)
    twin.observe_events(e2["src"], e2["dst"], e2["t"], e2["msg"], batch=16)
    assert tgn_epoch.observe(model, nl, e2["src"], e2["dst"], e2["t"], e2["msg"], batch=16) == (NEV + 120, 30)
    _assert_same_state(eng, twin, ctl=False)
    # and the train loop goes on over its bound split with the grown table (binding made again, graphs captured again)
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng.check()
