"""GPU tests of the live pair history in the TGN engine (TgnEngine.enable_pair_history) and of the
drop-in edgebank_stream / rank_stream(split_history=True).

Set-up: N = 40 (sources 0..19, destinations 20..39), 300 events, B = 50, mem_dim 2 and msg_dim 1 (the smallest widths
the engine takes), ring 10; source 0 meets 15 distinct destinations in the first 60 events and repeats later, so its
ring row (10 slots) no longer holds the oldest of them.  Parameters from a RefTGN state dict, dropout 0.

  seen           against PairHistory.build(rows).contains (the independent device implementation) on the 40 x 40 grid;
                 unchanged by compact_events() and grow_nodes(); pair_stats against the dict reference
  forget         no pair names the forgotten node afterwards, every other pair is kept
  queries        recommend_filtered / rank with exclude_history=True (similar through history_exclusions) equal, bit for
                 bit, the same calls with exclude= lists computed from the reference; exclude_seen alone lets an old
                 partner of source 0 through
  state          memory, stores and ring with the feature on equal an engine's with it off
  checkpoint     save_stream / load_stream carry the history; a file without one leaves it empty
  edgebank       edgebank_stream(window=None) equals edgebank_mrr exactly (600 events, K = 20); with a window it equals
                 the reference restatement
  split          rank_stream(split_history=True)'s parts against a recomputation from its ranks and the reference mask"""
import io
import types

import numpy as np
import pytest
import torch

import pairset_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, NEV, B, D, d, KN, RING = 40, 300, 50, 2, 1, 5, 10
_CACHE = {}


def _events(nev=NEV, seed=0):
    """A chronological bipartite stream with repeats; source 0 meets destinations 20..34 once each in its first 15
    events (spread over the first 60 rows), then only 30..34 again."""
    key = (nev, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        src, dst = rng.integers(1, 20, nev), rng.integers(20, 40, nev)
        rows = np.arange(0, 60, 4)
        src[rows], dst[rows] = 0, np.arange(20, 35)
        late = np.arange(100, nev, 9)
        src[late], dst[late] = 0, 30 + np.arange(late.size) % 5
        t = np.cumsum(rng.integers(0, 3, nev)).astype(np.float32)          # non-decreasing, with equal stamps
        _CACHE[key] = dict(src=src.astype(np.int64), dst=dst.astype(np.int64), t=t,
                           msg=rng.standard_normal((nev, d)).astype(np.float32))
    return _CACHE[key]


def _sd():
    from oracle.tgn_ref import RefTGN
    if "sd" not in _CACHE:
        torch.manual_seed(0)
        _CACHE["sd"] = RefTGN(N, d, hidden=D, dropout=0.0, layers=1, aggr="last").state_dict()
    return _CACHE["sd"]


def _model():
    from tgnx.tgn import TGNModel
    model = TGNModel(N, NEV, d, D, DEV, ring=RING, max_batch=B, max_neg=KN, dropout=0.0, layers=1, aggr="last")
    model.load_reference_state(_sd())
    return model


def _engine(ev=None, history=True):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine
    model = _model()
    eng = TgnEngine(model, LastNeighborLoader(N, RING, device=DEV), _events() if ev is None else ev,
                    TgnAdam(model, 1e-3), dst_nodes=np.arange(N), seed=7)
    eng.reset_state()
    eng.flush()
    if history:
        eng.enable_pair_history()
    return eng


def _ref(ev, lo=0, hi=None, n=N):
    ref = R.RefPairSet(n)
    ref.insert(ev["src"][lo:hi], ev["dst"][lo:hi], ev["t"][lo:hi])
    return ref


def _grid(n=N):
    s, c = np.divmod(np.arange(n * n), n)
    return s, c


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x.is_floating_point():
            x, y = torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)
        assert torch.equal(x, y)


def _lists(ref, src, cand, since=None):
    ptr, ids = ref.select(src, cand, since)
    return [ids[ptr[q]:ptr[q + 1]].tolist() for q in range(len(src))]


def test_seen_equals_the_static_index_and_survives_compaction_and_growth():
    from tgnx.tgb_negs import PairHistory
    ev, eng = _events(), _engine()
    eng.observe_range(0, NEV, B)
    gs, gc = _grid()
    want = PairHistory.build(ev["src"], ev["dst"], N, device=DEV).contains(gs, gc)
    assert int(want.sum()) > 100
    assert torch.equal(eng.seen(gs, gc), want)
    ref = _ref(ev)
    cnt, tf, tl = eng.pair_stats(gs, gc)
    _, wc, wf, wl = ref.lookup(gs, gc)
    assert np.array_equal(cnt.cpu().numpy(), wc) and np.array_equal(tf.cpu().numpy(), wf)
    assert np.array_equal(tl.cpu().numpy(), wl)
    mid = float(ev["t"][150])
    assert np.array_equal(eng.seen(gs, gc, since=mid).cpu().numpy(), ref.contains(gs, gc, mid))
    kept = eng.compact_events()
    assert kept.numel() < NEV                                   # rows were retired: the static index could not be rebuilt
    assert torch.equal(eng.seen(gs, gc), want)
    assert eng.grow_nodes(45) == 45
    assert torch.equal(eng.seen(gs, gc), want)
    g5, c5 = _grid(45)
    got = eng.seen(g5, c5).cpu().numpy()
    new = (g5 >= N) | (c5 >= N)
    assert not got[new].any() and int(got.sum()) == int(want.sum())
    eng.check()
    # recording goes on in the grown node space
    eng.observe_events([44, 0], [43, 20], [float(ev["t"][-1]) + 1] * 2, np.zeros((2, d), np.float32))
    assert eng.seen([44, 43], [43, 44]).tolist() == [True, False]
    assert int(eng.pair_stats([0], [20])[0]) == int(wc[0 * N + 20]) + 1


def test_reset_clear_record_and_disable():
    ev, eng = _events(), _engine()
    eng.observe_range(0, 100, B)
    assert eng._pairs.n_keys == _ref(ev, 0, 100).n_keys
    eng.clear_pair_history()
    assert eng._pairs.n_keys == 0
    eng.record_pairs(50, 200)
    R.assert_state_equal(eng.pair_history_state(), _ref(ev, 50, 200))
    eng.reset_state()
    assert eng._pairs.n_keys == 0 and not eng.seen([0], [20]).any()
    eng.eval_batch(0, B, torch.from_numpy(np.random.default_rng(0).integers(20, 40, (B, KN))))   # eval batches record
    R.assert_state_equal(eng.pair_history_state(), _ref(ev, 0, B))
    with pytest.raises(ValueError, match="record_pairs"):
        eng.record_pairs(0, NEV + 1)
    eng.disable_pair_history()
    for call in (lambda: eng.seen([0], [20]), lambda: eng.recommend_filtered([0], 3, exclude_history=True),
                 lambda: eng.rank([0], [20], exclude_history=True), lambda: eng.record_pairs(0, 1),
                 lambda: eng.history_exclusions([0]), lambda: eng.pair_history_state()):
        with pytest.raises(RuntimeError, match=r"enable_pair_history\(\)"):
            call()
    from tgnx.tgn import TgnEngine
    from tgnx.sampler import LastNeighborLoader
    model = _model()
    dp = TgnEngine(model, LastNeighborLoader(N, RING, device=DEV), ev, None, data_parallel=True)
    with pytest.raises(ValueError, match="one device only"):
        dp.enable_pair_history()


def test_forget_nodes_erases_the_pairs_that_name_the_node():
    ev, eng, off = _events(), _engine(), _engine(history=False)
    for e in (eng, off):
        e.observe_range(0, NEV, B)
    busiest = int(np.bincount(np.concatenate([ev["src"], ev["dst"]]), minlength=N).argmax())
    ref = _ref(ev)
    out = eng.forget_nodes([busiest])
    assert out["pairs"] == ref.erase([busiest]) > 0
    out_off = off.forget_nodes([busiest])
    assert "pairs" not in out_off and {k: v for k, v in out.items() if k != "pairs"} == out_off
    gs, gc = _grid()
    got = eng.seen(gs, gc).cpu().numpy()
    assert not got[(gs == busiest) | (gc == busiest)].any()
    assert np.array_equal(got, ref.contains(gs, gc))            # all others kept
    R.assert_state_equal(eng.pair_history_state(), ref)
    assert eng.forget_nodes([]) == dict(nodes=0, ring_slots=0, ring_rows=0, store_entries=0, pairs=0)


def test_exclude_history_equals_reference_exclude_lists():
    ev, eng = _events(), _engine()
    eng.observe_range(0, NEV, B)
    ref = _ref(ev)
    cand = np.arange(N)
    src = np.array([0, 3, 7, 25, 0])                             # 25 is a destination: no history as a source
    met0 = sorted(c for (s, c) in ref.map if s == 0)
    assert len(met0) == 15 > RING
    # exclude_seen alone lets an old partner of source 0 through; the history does not
    ring = set(eng.loader.neighbors[0][eng.loader.e_id[0] >= 0].tolist())
    old = set(met0) - ring
    assert old, "source 0's ring row still holds every partner"
    ids_seen = set(eng.recommend_filtered([0], N, exclude_seen=True)[1][0].tolist())
    assert old <= ids_seen
    ids_hist = set(eng.recommend_filtered([0], N, exclude_history=True)[1][0].tolist())
    assert not (set(met0) & ids_hist) and ids_hist - {-1} == set(cand.tolist()) - set(met0)
    lists = _lists(ref, src, cand)
    for kw in (dict(), dict(exclude_seen=True, exclude_self=True)):
        got = eng.recommend_filtered(src, 12, return_scores=True, exclude_history=True, **kw)
        want = eng.recommend_filtered(src, 12, return_scores=True, exclude=lists, **kw)
        _same(got, want)
    # a cut: only pairs last met at or after it
    mid = float(ev["t"][200])
    got = eng.recommend_filtered(src, 12, exclude_history=True, history_since=mid)
    _same(got, eng.recommend_filtered(src, 12, exclude=_lists(ref, src, cand, mid)))
    assert not all(torch.equal(a, b) for a, b in zip(got, eng.recommend_filtered(src, 12, exclude_history=True)))
    # a candidate subset with a duplicate
    sub = np.array([30, 21, 30, 39, 22, 31, 20])
    _same(eng.recommend_filtered(src, 4, candidates=sub, exclude_history=True),
          eng.recommend_filtered(src, 4, candidates=sub, exclude=_lists(ref, src, sub)))
    # per-source lists are filtered entry by entry
    per = [[20, 21, 30, 39], [25, 26], [22], [20], [34, 33, 22, 23, 34]]
    excl = [[c for c in row if (int(s), c) in ref.map] for s, row in zip(src, per)]
    _same(eng.recommend_filtered(src, 3, per_source=per, return_scores=True, exclude_history=True),
          eng.recommend_filtered(src, 3, per_source=per, return_scores=True, exclude=excl))
    # rank: the met candidates do not compete, the true destination still does
    rs, rd = ev["src"][250:300], ev["dst"][250:300]
    got = eng.rank(rs, rd, exclude_history=True)
    _same(got, eng.rank(rs, rd, exclude=_lists(ref, rs, cand)))
    assert not torch.equal(got[3], eng.rank(rs, rd)[3])          # fewer candidates were compared
    # similar keeps its signature: the history's lists go in as exclude=
    hp, hi = eng.history_exclusions(src)
    wp, wi = ref.select(src, cand)
    assert np.array_equal(hp.cpu().numpy(), wp) and np.array_equal(hi.cpu().numpy(), wi)
    _same(eng.similar(src, 6, candidates=cand, exclude=(hp, hi)), eng.similar(src, 6, candidates=cand, exclude=lists))
    eng.check()


def test_calls_without_the_history_prepare_their_candidates_once():
    """With nothing excluded recommend_filtered is recommend(): the candidates are made once, by _recommend, as before
    the history existed; with exclusions once too."""
    eng = _engine(history=False)
    eng.observe_range(0, 100, B)
    calls, inner = [], eng._candidates
    eng._candidates = lambda c: (calls.append(1), inner(c))[1]
    eng.recommend_filtered([0, 3], 5)
    assert len(calls) == 1
    eng.recommend_filtered([0, 3], 5, exclude_seen=True)
    assert len(calls) == 2
    eng.enable_pair_history()
    eng.recommend_filtered([0, 3], 5, exclude_history=True)
    assert len(calls) == 3


def test_stream_state_is_that_of_an_engine_without_the_feature():
    on, off = _engine(), _engine(history=False)
    for e in (on, off):
        e.observe_range(0, NEV, B)
        e.check()
    for a, b in ((on.model.memory.memory, off.model.memory.memory), (on.model.store, off.model.store),
                 (on.model.memory.last_update, off.model.memory.last_update), (on.model.node_gen, off.model.node_gen),
                 (on.loader.neighbors, off.loader.neighbors), (on.loader.e_id, off.loader.e_id),
                 (on.loader.t, off.loader.t), (on.ctl, off.ctl)):
        assert torch.equal(a, b)
    ps = on._pairs                                                # from next_pow2(8 * B) = 512 slots; load <= 1/2, and
    assert ps.capacity >= 512 and ps.n_keys <= ps.capacity // 2   # host reads >= capacity / 8 recorded events apart
    assert ps.reads <= NEV // (512 // 8)


def test_checkpoint_round_trip_through_save_stream_and_load_stream():
    import pyg_epoch_utils
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam
    ev, a = _events(), _engine()
    a.observe_range(0, NEV, B)
    a.model._tgnx_engine, a._mode_train, a._bound = a, False, (0, NEV, B)      # as train() / test() attach it
    assert pyg_epoch_utils.seen(a.model, a.loader, [0], [20]).tolist() == [True]
    f = io.BytesIO()
    pyg_epoch_utils.save_stream(a.model, a.loader, f)
    f.seek(0)
    state = torch.load(f, map_location="cpu")
    from tgnx.tgn import STREAM_STATE_FORMAT
    assert state["format"] == STREAM_STATE_FORMAT and set(state) - set(a.stream_state()) == {"pair_history"}
    f.seek(0)
    model, nl = _model(), LastNeighborLoader(N, RING, device=DEV)
    pyg_epoch_utils.load_stream(model, nl, f, optimizer=TgnAdam(model, 1e-3), dst_nodes=np.arange(N))
    c = model._tgnx_engine
    R.assert_state_equal(c.pair_history_state(), _ref(ev))
    c.load_stream_state(state)                                   # the engine call takes the file's dict as it is
    assert c.num_events == a.num_events
    R.assert_state_equal(c.pair_history_state(), _ref(ev))       # (and leaves the history alone)
    gs, gc = _grid()
    assert torch.equal(c.seen(gs, gc), a.seen(gs, gc))
    _same(c.recommend_filtered([0, 3], 5, exclude_history=True), a.recommend_filtered([0, 3], 5, exclude_history=True))
    # a file without a history: an enabled history is left empty
    b = _engine(history=False)
    b.observe_range(0, 100, B)
    b.model._tgnx_engine, b._mode_train, b._bound = b, False, (0, 100, B)
    f = io.BytesIO()
    pyg_epoch_utils.save_stream(b.model, b.loader, f)
    f.seek(0)
    assert "pair_history" not in torch.load(f, map_location="cpu")
    f.seek(0)
    pyg_epoch_utils.load_stream(a.model, a.loader, f)
    assert a._pairs is not None and a._pairs.n_keys == 0 and a.num_events == b.num_events


def _bank_stream():
    ev = _events(600, seed=1)
    data = types.SimpleNamespace(src=torch.from_numpy(ev["src"]), dst=torch.from_numpy(ev["dst"]),
                                 t=torch.from_numpy(ev["t"]))
    negs = np.random.default_rng(2).integers(20, 40, (300, 20))
    return ev, data, negs


def test_edgebank_stream_inf_equals_edgebank_mrr():
    import pyg_epoch_utils
    from tgnx.tgb_negs import PairHistory, edgebank_mrr
    ev, data, negs = _bank_stream()
    lo, hi = 300, 600
    idx = PairHistory.build(ev["src"], ev["dst"], N, device=DEV)
    for batch in (50, 64):
        want = edgebank_mrr(idx, ev["src"], ev["dst"], negs, lo, hi, batch)
        got = pyg_epoch_utils.edgebank_stream(data, lo, hi, batch, negs)
        print(f"batch {batch}: edgebank_stream {got!r} edgebank_mrr {want!r}")
        assert got == want and 0.0 < got < 1.0
        assert got == R.edgebank_stream_ref(ev["src"], ev["dst"], ev["t"], lo, hi, batch, negs)


def test_edgebank_stream_window_equals_the_reference():
    import pyg_epoch_utils
    ev, data, negs = _bank_stream()
    lo, hi = 300, 600
    inf = pyg_epoch_utils.edgebank_stream(data, lo, hi, 50, negs)
    span = float(ev["t"][lo - 1] - ev["t"][0])
    assert pyg_epoch_utils.edgebank_window(ev["t"][:lo]) == pytest.approx(0.15 * span)
    seen = set()
    for window in (pyg_epoch_utils.edgebank_window(ev["t"][:lo]), 0.0, 40.0, 10.0 * span):
        got = pyg_epoch_utils.edgebank_stream(data, lo, hi, 50, negs, window=window)
        want = R.edgebank_stream_ref(ev["src"], ev["dst"], ev["t"], lo, hi, 50, negs, window=window)
        print(f"window {window}: edgebank_stream {got!r} reference {want!r}")
        assert got == want
        seen.add(got)
    assert got == inf and len(seen) > 2                          # a window longer than the stream is EdgeBank-inf
    # from an empty bank (lo = 0) the first batch scores nothing
    got = pyg_epoch_utils.edgebank_stream(data, 0, 300, 50, negs, window=5.0)
    assert got == R.edgebank_stream_ref(ev["src"], ev["dst"], ev["t"], 0, 300, 50, negs, window=5.0)


def test_rank_stream_split_history():
    import pyg_epoch_utils
    ev = _events()
    lo, hi, ks = 100, NEV, (1, 3, 10)
    mask = R.repeat_mask(ev["src"], ev["dst"], ev["t"], lo, hi, B)
    assert mask.any() and (~mask).any()                          # the stream has both parts
    eng, twin = _engine(), _engine(history=False)
    for e in (eng, twin):
        e.observe_range(0, lo, B)
        e.model._tgnx_engine, e._mode_train, e._bound = e, False, (0, NEV, B)
    with pytest.raises(RuntimeError, match=r"enable_pair_history\(\)"):
        pyg_epoch_utils.rank_stream(twin.model, twin.loader, lo, hi, B, ks=ks, split_history=True)
    out = pyg_epoch_utils.rank_stream(eng.model, eng.loader, lo, hi, B, ks=ks, split_history=True)
    plain = pyg_epoch_utils.rank_stream(twin.model, twin.loader, lo, hi, B, ks=ks)
    assert torch.equal(out["rank"], plain["rank"])
    for k in plain:                                              # existing keys and values unchanged
        if k != "rank":
            assert out[k] == plain[k], k
    assert np.array_equal(out["repeat"].cpu().numpy(), mask)
    assert out["n_repeat"] == int(mask.sum()) and out["n_repeat"] + out["n_novel"] == hi - lo
    # the existing keys by the expression rank_stream had before the split existed, on the returned ranks
    r = out["rank"]
    want = torch.stack([torch.nan_to_num(1.0 / r, nan=0.0).sum()] + [(r <= k).sum().double() for k in ks])
    want = (want / max(hi - lo, 1)).tolist()
    assert out["mrr"] == want[0] and [out[f"hits@{k}"] for k in ks] == want[1:]
    # the parts: numpy means over the part's ranks, exactly
    rank = r.cpu().numpy()
    for name, m in (("repeat", mask), ("novel", ~mask)):
        assert out[f"mrr_{name}"] == float(np.mean(1.0 / rank[m]))
        for k in ks:
            assert out[f"hits@{k}_{name}"] == float(np.mean(rank[m] <= k))
    print({k: v for k, v in out.items() if not torch.is_tensor(v)})
    # the history went on recording through rank_events
    R.assert_state_equal(eng.pair_history_state(), _ref(ev))
    # with the history excluded a repeat's rivals shrink: its rank cannot get worse
    eng2 = _engine()
    eng2.observe_range(0, lo, B)
    eng2.model._tgnx_engine, eng2._mode_train, eng2._bound = eng2, False, (0, NEV, B)
    ex = pyg_epoch_utils.rank_stream(eng2.model, eng2.loader, lo, hi, B, ks=ks, exclude_history=True)
    assert bool((ex["rank"] <= out["rank"]).all()) and bool((ex["rank"] < out["rank"]).any())
