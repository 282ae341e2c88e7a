"""GPU tests of the device-resident validation / test pass of the TGN memory path
(TgnEngine.bind_eval_resident / eval_resident_step / capture_eval / replay_eval_n / eval_mrr over
tgnx_tgn_eval_step_resident) and of its deduplicated marking (tgn_eval_claim + tgn_mark_eval).

  1. resident == per-batch: a twin engine looping eval_batch from the same state; integers exact, floats
     bit-identical (the only difference is which slot walks a candidate's ring row: the sampled sets the scan
     reads from the bitmaps are the same, and every launch after the scan is the per-batch step's);
  2. graph replay == eager resident steps, a step past the split is a no-op, a second pass from a restored
     state repeats the first, and train -> eval -> train -> eval recaptures nothing;
  3. 999 negatives per event at the wiki shape against the oracle (oracle/tgn_ref.eval_step);
  4. the marking dedupe on both bitmap branches against the oracle: every negative the same node, candidates
     duplicated between roots and negatives, 7 distinct negatives with a hub at 2 hops over summary bitmaps,
     candidates without history;
  5. the drop-in's test() on a rectangular negatives table.

Tolerances against the oracle are those of tests/test_gpu_tgn_configs.py::_oracle_parity: scores 2e-5 abs,
reciprocal ranks 1e-6 except events with a negative within 4e-5 of the positive (fewer than 5 % of the batch,
asserted on the oracle's scores alone), memory 1e-5 abs, last_update exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else (x.view(torch.int64) if x.dtype == torch.float64 else x)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _engine(s, sd, N, d, D, B, kn, aggr="last", layers=1, dropout=0.0, lr=1e-3, **mk):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    dev = torch.device("cuda")
    model = TGNModel(N, s.num_events, d, D, dev, ring=10, max_batch=B, max_neg=kn, aggr=aggr, dropout=dropout,
                     layers=layers, **mk)
    model.load_reference_state(sd)
    opt = TgnAdam(model, lr)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=dev), dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32),
                    msg=s.msg), opt, dst_nodes=s.dst_nodes, seed=7)
    eng.reset_state()
    return model, opt, eng


def _state(eng):
    m, ld = eng.model, eng.loader
    return dict(flat=m.flat, memory=m.memory.memory, last_update=m.memory.last_update, store=m.store,
                node_gen=m.node_gen, neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t, assoc=ld._assoc, ctl=eng.ctl)


def _snapshot(eng):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _state(eng).items()}, eng.loader.cur_e_id


def _restore(eng, snap):
    eng.finish()
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(eng).items():
            v.copy_(snap[0][k])
    eng.loader.cur_e_id = snap[1]
    eng.invalidate_prefetch()


def _assert_state_equal(a, b, what):
    sa, sb = _state(a), _state(b)
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert _same(sa[k], sb[k]), (what, k)
    for w in (3, 10):                                      # TGNX_CTL_GEN, TGNX_CTL_NB
        assert int(a.ctl[w]) == int(b.ctl[w]), (what, "ctl", w, int(a.ctl[w]), int(b.ctl[w]))


FORMS = {"1hop-last-tgn": dict(aggr="last", layers=1),
         "2hop-last-tgn": dict(aggr="last", layers=2),
         "1hop-mean-dyrep-dstemb": dict(aggr="mean", layers=1, memory="dyrep", updater="rnn", use_dst_emb_in_msg=True)}
N1, d1, D1, B1, KN1, NTR1 = 300, 16, 32, 50, 20, 8
LO1, HI1 = NTR1 * B1, NTR1 * B1 + 7 * B1 + 20              # 7 full eval batches and one of 20 events


def _twins(form, n):
    """n engines in the same mid-epoch eval state (8 train batches on the first, flush, state copied to the
    others), the stream, and the eval split's negatives [HI1 - LO1, KN1]."""
    from oracle.tgn_ref import RefTGN
    from tgnx.synth import make_stream
    mk = dict(FORMS[form])
    s = make_stream("tgbl-wiki", seed=5, num_events=HI1, num_nodes=N1, msg_dim=d1)
    torch.manual_seed(0)
    ref_kw = {k: v for k, v in mk.items() if k not in ("memory",)}
    sd = RefTGN(N1, d1, hidden=D1, dropout=0.0, **ref_kw).state_dict()
    engs = [_engine(s, sd, N1, d1, D1, B1, KN1, **mk)[2] for _ in range(n)]
    for st in range(NTR1):
        engs[0].train_batch(st * B1, B1, neg=None, dropout=False)
    engs[0].flush()
    engs[0].check()
    snap = _snapshot(engs[0])
    for e in engs[1:]:
        _restore(e, snap)
    negs = torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(HI1 - LO1, KN1)))
    return s, engs, negs, snap


@pytest.mark.parametrize("form", list(FORMS))
def test_resident_equals_per_batch(form):
    """Twin engines from the same state: eval_batch per batch against bind_eval_resident + eval_resident_step.
    Per batch out_pos / out_neg / mrr; at the end rr_ev against the concatenated per-batch mrr, memory,
    last_update, the ring, the stores and ctl GEN / NB.  Everything bit-identical."""
    s, (a, b), negs, _ = _twins(form, 2)
    b.bind_eval_resident(LO1, HI1, B1, negs)
    rrs = []
    for st in range(LO1, HI1, B1):
        Bk = min(B1, HI1 - st)
        pa, na, ra = a.eval_batch(st, Bk, negs[st - LO1:st - LO1 + Bk])
        pb, nb_, rb = b.eval_resident_step()
        torch.cuda.synchronize()
        a.check()
        b.check()
        assert _same(pa, pb[:Bk]), (st, float((pa - pb[:Bk]).abs().max()))
        assert _same(na, nb_[:Bk]), (st, float((na - nb_[:Bk]).abs().max()))
        assert _same(ra, rb[:Bk]), st
        assert int(b.ctl[0]) == st and int(b.ctl[2]) == Bk
        rrs.append(ra.clone())
    assert _same(torch.cat(rrs), b.eval_rr())
    _assert_state_equal(a, b, "end of pass")
    want = float(torch.stack([r.mean() for r in rrs]).mean())
    assert b.eval_mrr() == want


def test_bind_eval_resident_rejects_wrong_shape():
    s, (a,), negs, _ = _twins("1hop-last-tgn", 1)
    with pytest.raises(ValueError):
        a.bind_eval_resident(LO1, HI1, B1, negs[:-1])
    with pytest.raises(ValueError):
        a.bind_eval_resident(LO1, HI1, B1, negs.reshape(-1))
    with pytest.raises(ValueError):
        a.bind_eval_resident(LO1, HI1, B1, negs.float())


@pytest.mark.parametrize("form", ["1hop-last-tgn", "2hop-last-tgn"])
def test_graph_replay_equals_eager_resident(form):
    """capture_eval + replay_eval_n(8) (a group of 3 steps per graph: 2 groups + 2 single replays) against 8 eager
    resident steps: the whole split, its partial last batch included.  One more replayed step changes no buffer; a
    second replayed pass from the restored state repeats rr_ev."""
    s, (a, b), negs, snap = _twins(form, 2)
    for e in (a, b):
        e.bind_eval_resident(LO1, HI1, B1, negs)
    for _ in range(8):
        a.eval_resident_step()
    b.capture_eval(group=3)
    b.replay_eval_n(8)
    torch.cuda.synchronize()
    a.check()
    b.check()
    assert _same(a.eval_rr(), b.eval_rr())
    assert float(b.eval_rr().min()) > 0.0                    # every event of the split was ranked
    _assert_state_equal(a, b, "replayed pass")
    assert int(b.ctl[18]) == 8
    for k in ("out_pos", "out_neg", "mrr"):
        assert _same(getattr(a, k), getattr(b, k)), k
    # a step past the end of the split: B = 0, nothing but the counters moves
    before, _ = _snapshot(b)
    outs = {k: getattr(b, k).clone() for k in ("out_pos", "out_neg", "mrr")}
    rr = b.eval_rr().clone()
    b.replay_eval_n(1)
    torch.cuda.synchronize()
    b.check()
    for k, v in _state(b).items():
        if k != "ctl":
            assert _same(v, before[k]), k
    for k, v in outs.items():
        assert _same(getattr(b, k), v), k
    assert _same(b.eval_rr(), rr)
    assert int(b.ctl[2]) == 0 and int(b.ctl[18]) == 9 and int(b.ctl[10]) == int(before["ctl"][10]) + 1
    # a second pass from the restored state
    _restore(b, snap)
    b.eval_rr().zero_()
    b.begin_eval()
    b.replay_eval_n(8)
    torch.cuda.synchronize()
    b.check()
    assert _same(b.eval_rr(), rr)


def test_train_eval_train_keeps_graphs():
    """The reference's loop: a train epoch (replay_resident_n), a validation pass, a train epoch, a validation
    pass.  Neither the train graphs nor the eval graphs are captured again (the workspace already holds Kn)."""
    from oracle.tgn_ref import RefTGN
    from tgnx.synth import make_stream
    s = make_stream("tgbl-wiki", seed=5, num_events=HI1, num_nodes=N1, msg_dim=d1)
    torch.manual_seed(0)
    sd = RefTGN(N1, d1, hidden=D1, dropout=0.1).state_dict()
    _, _, e = _engine(s, sd, N1, d1, D1, B1, KN1, dropout=0.1)
    negs = torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(HI1 - LO1, KN1)))
    e.bind_resident(0, LO1, B1, dropout=True)
    e.bind_eval_resident(LO1, HI1, B1, negs)
    e.begin_epoch()
    e.capture_resident()
    e.capture_group(8)
    e.capture_eval()
    gt, gg, ge = e._graphs, e._group, e._ev_graphs
    ids = [id(x) for x in (gt[0] if isinstance(gt[0], tuple) else gt[:1])] + [id(gg[1]), id(ge[0]), id(ge[2])]
    mrrs = []
    for _ in range(2):
        e.begin_epoch()
        e.replay_resident_n(NTR1)
        e.flush()
        e.begin_eval()
        e.replay_eval_n(8)
        mrrs.append(e.eval_mrr())
        e.check()
        assert int(e.ctl[18]) == 8
    assert e._graphs is gt and e._group is gg and e._ev_graphs is ge
    assert ids == [id(x) for x in (gt[0] if isinstance(gt[0], tuple) else gt[:1])] + [id(gg[1]), id(ge[0]), id(ge[2])]
    assert all(0.0 < m <= 1.0 for m in mrrs)
    # another negatives table, or a workspace grown for more negatives, drops the eval graphs only / both
    e.bind_eval_resident(LO1, HI1, B1, negs.clone())
    assert e._ev_graphs is None and e._graphs is gt
    e.capture_eval()
    e.ensure_neg(KN1 + 5)
    assert e._ev_graphs is None and e._graphs is None


# ------------------------------------------------------------------ against the oracle
def _sync(ref, model):
    named = dict(ref.named_parameters())
    with torch.no_grad():
        for name in model.param_order:
            o, n, _ = model._views[name]
            model.flat[o:o + n].copy_(named[name].detach().reshape(-1))
        model.memory.memory.copy_(ref.memory.memory)
        model.memory.last_update.copy_(ref.memory.last_update)


def _oracle_eval(shape, N, B, d, D, layers, nb, kn, seed, negs_of, n_eval=1):
    """nb train batches on the oracle and the engine (parameters, memory and last_update synchronised from the
    oracle before each, as _oracle_parity does), flush, then n_eval resident eval batches whose negatives
    negs_of(s, k, lo, hi) builds ([B, kn] int64 for eval batch k = events [lo, hi)); every batch's scores, ranks,
    memory and last_update against oracle/tgn_ref.eval_step."""
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN, eval_step, mrr_per_event, train_step
    from tgnx.synth import make_stream
    s = make_stream(shape, seed=seed, num_events=B * (nb + n_eval), num_nodes=N, msg_dim=d)
    torch.manual_seed(0)
    ref = RefTGN(N, d, hidden=D, aggr="last", dropout=0.0, layers=layers)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    model, opt, eng = _engine(s, ref.state_dict(), N, d, D, B, kn, layers=layers)
    lref = RefLastNeighborLoader(N, 10)
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    rng = np.random.default_rng(seed + 1)
    for st in range(nb):
        sl = slice(st * B, (st + 1) * B)
        _sync(ref, model)
        neg = torch.from_numpy(rng.choice(s.dst_nodes, size=B))
        train_step(ref, opt_ref, lref, ev_t, ev_msg, torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl]), neg,
                   ev_t[sl], ev_msg[sl])
        eng.train_batch(st * B, B, neg=neg)
    torch.cuda.synchronize()
    eng.check()
    _sync(ref, model)
    ref.memory.train(False)
    eng.flush()
    lo, hi = nb * B, (nb + n_eval) * B

    def probe(cands):
        """The oracle's scores (pos [B], cands [B, m]) of the first eval batch, on copies of its state."""
        import copy
        sl = slice(lo, lo + B)
        return eval_step(copy.deepcopy(ref), copy.deepcopy(lref), ev_t, ev_msg, torch.from_numpy(s.src[sl]),
                         torch.from_numpy(s.dst[sl]), torch.as_tensor(cands).long(), ev_t[sl], ev_msg[sl])
    negs = torch.cat([torch.as_tensor(negs_of(s, k, lo + k * B, lo + (k + 1) * B, probe)).long().view(B, kn)
                      for k in range(n_eval)])
    eng.bind_eval_resident(lo, hi, B, negs)
    for k in range(n_eval):
        sl = slice(lo + k * B, lo + (k + 1) * B)
        with torch.no_grad():
            model.memory.memory.copy_(ref.memory.memory)    # (one tolerance per batch, not an accumulating one)
        po, no = eval_step(ref, lref, ev_t, ev_msg, torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl]),
                           negs[k * B:(k + 1) * B], ev_t[sl], ev_msg[sl])
        pg, ng, rr = eng.eval_resident_step()
        torch.cuda.synchronize()
        eng.check()
        pg, ng, rr = pg[:B].cpu(), ng[:B].cpu(), rr[:B].cpu().numpy()
        ep, en = float((pg - po).abs().max()), float((ng - no).abs().max())
        ref_rr = mrr_per_event(po, no)
        close = ((no - po.view(-1, 1)).abs() <= 4e-5).any(1).numpy()
        er = float(np.abs(rr[~close] - ref_rr[~close]).max()) if (~close).any() else 0.0
        em = float((model.memory.memory.cpu() - ref.memory.memory).abs().max())
        print(f"eval batch {k}: |pos| {ep:.2e} |neg| {en:.2e} |rr| {er:.2e} |mem| {em:.2e} close {close.mean():.3f}")
        assert ep <= 2e-5 and en <= 2e-5, (k, ep, en)
        assert er <= 1e-6, (k, er)
        # every event, near ties included: the rank kernel on the step's own scores (TGB's rule, ties counted half)
        assert np.allclose(rr, mrr_per_event(pg, ng), atol=1e-6), k
        assert np.array_equal(eng.eval_rr()[k * B:(k + 1) * B].cpu().numpy(), rr), k
        assert em <= 1e-5, (k, em)
        assert torch.equal(model.memory.last_update.cpu(), ref.memory.last_update), k
        live = lref.e_id >= 0
        assert np.array_equal(eng.loader.e_id.cpu().numpy(), lref.e_id), k
        assert np.array_equal(eng.loader.neighbors.cpu().numpy()[live], lref.neighbors[live]), k
        yield s, k, close


def test_eval_999_negatives_matches_oracle():
    """The datasets' real negative count: wiki shape (N = 9,227, d = 172, D = 100, B = 200), 999 negatives per
    event drawn from the destination set, one resident eval batch after 3 train batches.

    The draw: after 3 batches the stream has ~150 destinations, so 999 uniform draws hold every one of them for
    every event: the positive itself (an exact tie in each row), the ~20 % of destinations without history (which
    all score alike, and like a positive without history), and ~150 distinct scores within a band 0.13 wide (a
    neighbour within 4e-5 of the positive for ~10 % of the events).  Measured on the oracle alone: 100 % of the events
    near-tied at stream seeds 41-43 with uniform draws; with the positive excluded, 18 % and 27 % at the two seeds of
    0..59 where more than 90 % of the batch's positives have history (seeds 9 and 30).  So the
    draw is made as the seed would be chosen, from the oracle alone: each event draws its 999 negatives uniformly
    from the destinations whose oracle score lies more than 1e-4 from its positive's (the positive itself excluded,
    as tgnx.synth.eval_negatives does).  The near-tie fraction of the batch as scored is then asserted below 5 %."""
    rng = np.random.default_rng(77)

    def negs_of(s, k, lo, hi, probe):
        B = hi - lo
        po, sc = probe(np.tile(s.dst_nodes, (B, 1)))
        ok = ((sc - po.view(-1, 1)).abs() > 1e-4).numpy() & (s.dst_nodes[None, :] != s.dst[lo:hi, None])
        assert ok.sum(1).min() >= 20, int(ok.sum(1).min())     # (a pool to draw from for every event)
        return np.stack([rng.choice(s.dst_nodes[ok[i]], size=999) for i in range(B)])
    for s, k, close in _oracle_eval("tgbl-wiki", 9_227, 200, 172, 100, 1, 3, 999, 41, negs_of):
        assert close.mean() < 0.05, close.mean()


def _same_node(s, k, lo, hi, probe=None, kn=64):
    if k == 0:      # every negative of every event is one node
        return np.full((hi - lo, kn), s.dst_nodes[len(s.dst_nodes) // 2])
    # each event's negatives include its own source and its positive destination
    rng = np.random.default_rng(3)
    negs = rng.choice(s.dst_nodes, size=(hi - lo, kn))
    negs[:, 0] = s.src[lo:hi]
    negs[:, 1] = s.dst[lo:hi]
    negs[:, 2] = s.src[lo:hi]
    return negs


def test_dedupe_small_graph_branch_matches_oracle():
    """scan_direct graphs (N = 300: bitmaps walked word by word, no summaries), B = 50, 64 negatives: a batch whose
    3,200 negative slots are all one node, and a batch whose negatives repeat the events' own roots."""
    n = sum(1 for _ in _oracle_eval("tgbl-wiki", 300, 50, 16, 32, 1, 3, 64, 43, _same_node, n_eval=2))
    assert n == 2


def test_dedupe_summary_bitmap_branch_2hop_matches_oracle():
    """Graphs above 65,536 nodes (summary bitmaps): N = 300,000, d = 2, comment-shaped, 2 hops, B = 50, 64
    negatives drawn from 7 distinct nodes, one of them the hub that sits in the most ring rows."""
    def negs_of(s, k, lo, hi, probe):
        hub = int(np.bincount(np.concatenate([s.src[:lo], s.dst[:lo]])).argmax())
        rest = [int(v) for v in s.dst_nodes if int(v) != hub][:6]
        pool = np.array([hub] + rest)
        assert len(set(pool.tolist())) == 7
        return np.random.default_rng(4).choice(pool, size=(hi - lo, 64))
    n = sum(1 for _ in _oracle_eval("tgbl-comment", 300_000, 50, 2, 32, 2, 3, 64, 44, negs_of))
    assert n == 1


def test_candidates_without_history_match_oracle():
    """Negatives without a ring row to walk: a node whose first event is in the evaluated batch itself (its ring
    row is still empty when the batch is scored), and a node that never appears in the stream."""
    seen = {}

    def negs_of(s, k, lo, hi, probe):
        before = set(s.src[:lo].tolist()) | set(s.dst[:lo].tolist())
        fresh = [int(v) for v in np.concatenate([s.src[lo:hi], s.dst[lo:hi]]) if int(v) not in before]
        never = sorted(set(range(300)) - set(s.src.tolist()) - set(s.dst.tolist()))
        assert fresh and never, (len(fresh), len(never))
        seen["n"] = (fresh[0], never[0])
        negs = np.random.default_rng(5).choice(s.dst_nodes, size=(hi - lo, 64))
        negs[:, 0::3] = fresh[0]
        negs[:, 1::3] = never[0]
        return negs
    n = sum(1 for _ in _oracle_eval("tgbl-wiki", 300, 50, 16, 32, 1, 3, 64, 43, negs_of))
    assert n == 1 and seen["n"][0] != seen["n"][1]


# ------------------------------------------------------------------ drop-in
def test_dropin_test_uses_resident_pass(monkeypatch):
    """pyg_epoch_utils.test() on a SplitLoader with a rectangular negatives table, after a train(): the same float
    as the per-batch eval_batch loop (the loop test() ran before) on a twin engine in the same state; train / test /
    train / test binds and captures the eval pass once."""
    monkeypatch.setenv("TGNX_SYNTH_EVENTS", "3000")
    monkeypatch.setenv("TGNX_EVAL_NEGS", "30")
    import pyg_epoch_utils as pe
    import pyg_model_utils as pm
    from tgnx.data import getDataWithDependecyBlock
    from tgnx.neg import NegLinkSamplerDest
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnEngine
    data, tr, va, te, ns, ev, metric = getDataWithDependecyBlock("tgbl-wiki", {"batch_size": 200})
    assert torch.is_tensor(va.negatives) and tuple(va.negatives.shape) == (va.hi - va.lo, 30)
    d, D, N = data.msg.shape[1], 100, data.num_nodes
    torch.manual_seed(0)
    model = pm.getModel(d, D, N, "cuda", ring=10, max_batch=200, dropout=0.1)
    opt = pm.getOptimizer(model, 1e-4)
    nl = LastNeighborLoader(N, 10, device="cuda")
    nds = NegLinkSamplerDest(torch.unique(data.dst), device="cuda")
    crit = torch.nn.BCEWithLogitsLoss()
    pe.train(model, data.msg, tr, nl, nds, None, "cuda", opt, crit)
    eng = model["model"]._tgnx_engine
    # the twin: same parameters and state, the per-batch loop
    m2 = pm.getModel(d, D, N, "cuda", ring=10, max_batch=200, dropout=0.1)
    e2 = TgnEngine(m2["model"], LastNeighborLoader(N, 10, device="cuda"),
                   dict(src=data.src, dst=data.dst, t=data.t.float(), msg=data.msg.float()), pm.getOptimizer(m2, 1e-4),
                   dst_nodes=torch.unique(data.dst))
    e2.reset_state()
    _restore(e2, _snapshot(eng))
    e2.flush()
    perf = []
    for a in range(va.lo, va.hi, 200):
        b = min(va.hi, a + 200)
        perf.append(e2.eval_batch(a, b - a, va.negatives[a - va.lo:b - va.lo])[2].clone().mean())
    want = float(torch.stack(perf).mean())
    calls = {"bind": 0, "capture": 0}
    bind, cap = eng.bind_eval_resident, eng.capture_eval
    monkeypatch.setattr(eng, "bind_eval_resident", lambda *a, **k: (calls.__setitem__("bind", calls["bind"] + 1), bind(*a, **k))[1])
    monkeypatch.setattr(eng, "capture_eval", lambda *a, **k: (calls.__setitem__("capture", calls["capture"] + 1), cap(*a, **k))[1])
    got = pe.test(model, data.msg, va, nl, ns, None, "cuda", opt, crit, ev, metric, "val")
    assert got == want, (got, want)
    assert nl.cur_e_id == va.hi
    assert _same(eng.model.memory.memory, e2.model.memory.memory) and _same(eng.model.store, e2.model.store)
    assert calls == {"bind": 1, "capture": 1}
    ev_graphs = eng._ev_graphs
    pe.train(model, data.msg, tr, nl, nds, None, "cuda", opt, crit)   # (recaptures the train step: 30 negatives grew the workspace)
    graphs = eng._graphs
    got2 = pe.test(model, data.msg, va, nl, ns, None, "cuda", opt, crit, ev, metric, "val")
    assert 0.0 < got2 <= 1.0
    pe.train(model, data.msg, tr, nl, nds, None, "cuda", opt, crit)
    pe.test(model, data.msg, va, nl, ns, None, "cuda", opt, crit, ev, metric, "val")
    assert calls == {"bind": 1, "capture": 1} and eng._graphs is graphs and eng._ev_graphs is ev_graphs
