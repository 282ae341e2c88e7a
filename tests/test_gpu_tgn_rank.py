"""GPU tests of full-catalogue link ranking on the engine: TgnEngine.rank / rank_events over embed(), the fused rank
operator and observe(), and the drop-in tgn_epoch.rank_stream.

Setup: tests/test_gpu_tgn_query.py's — the 600-event stream over 300 nodes, D = 32, six eval batches of 50 on the
engine and on the oracle, layers in {1, 2} x aggr in {last, mean}.  The ranked pairs are the 50 events of the batch
after the six evaluated ones, src[e] -> dst[e], against the engine's destination set.

  exact      (gt, eq, n, rank) equal tests/link_rank_ref.py on the logits the same call returns (every destination of
             the stream is a candidate, and a node embedded twice in one call has one row, so the target's logit is
             the column of its node);
  oracle     with tol = 2e-5, scale = max(|ref|, 1) and r the oracle's all-pairs logits over the compared set:
             #{r > r_t + 2 tol scale} <= gt and gt + eq <= #{r >= r_t - 2 tol scale}.  The two bounds coincide on the
             oracle alone for 49, 46, 49 and 49 of the 50 rows in the four forms (checked on the CPU; asserted >= 9 in
             10 here); prob within 2e-5 of eng.score(src, dst);
  filters    exclude_seen never raises gt or n and lowers gt where the oracle puts a seen candidate above the target
             by more than 2 tol scale; a target inside its source's ring row is still ranked; an empty ring row
             changes nothing; exclude_self; a destination outside `candidates` is ranked against all of them;
  read-only  memory, last_update, stores, ring, parameters, moments and every ctl word but GEN bit-identical;
  rank_events    equals rank() on a twin bit for bit, and leaves the state of a twin that only observed (node_gen,
                 the per-node generation stamps, holds the GEN word that rank()'s embed calls advanced: the same
                 nodes carry the latest stamp, every older stamp is equal);
  rank_stream    equals the hand loop on a twin, mrr / hits@k recomputed from the returned ranks, one flush."""
import numpy as np
import pytest
import torch

from link_rank_ref import link_rank_ref
from test_gpu_tgn_query import (B, DEV, FORMS, KN, N, NEV, TOL, _bits, _built, _close, _engine, _eval_batches, _negs,
                                _ref, _state, _stream)
from test_gpu_tgn_recommend_filtered import NS, _oracle_logits, _ring, _sources
from topk_filter_ref import seen_lists

pytestmark = pytest.mark.gpu
E0 = 6 * B                                                             # the first event after the evaluated ones


def _np(out):
    return [t.cpu().numpy() for t in out]


def _bounds(ref, key, C, skey=None, ptr=None, keys=None):
    """Per row q of the oracle's logits ref [Q, C + Q] (target of q: column C + q):
    (#{r > r_t + 2 tol scale}, #{r >= r_t - 2 tol scale}) over the compared set, and the set's size."""
    ref = np.asarray(ref, dtype=np.float64)
    m = 2 * TOL * max(float(np.abs(ref).max()), 1.0)
    out = []
    for q in range(ref.shape[0]):
        ok = key[:C] != key[C + q]
        if skey is not None:
            ok &= key[:C] != skey[q]
        if ptr is not None:
            ok &= ~np.isin(key[:C], keys[ptr[q]:ptr[q + 1]])
        r, rt = ref[q, :C][ok], ref[q, C + q]
        out.append((int((r > rt + m).sum()), int((r >= rt - m).sum()), int(ok.sum())))
    return out, m


def _check_bracket(gt, eq, n, bounds, share=True):
    sharp = 0
    for q, (lo, hi, size) in enumerate(bounds):
        assert lo <= gt[q] and gt[q] + eq[q] <= hi, (q, lo, gt[q], eq[q], hi)
        assert n[q] == size, (q, n[q], size)
        sharp += lo == hi
    print(f"bounds coincide on {sharp} of {len(bounds)} rows")
    if share:
        assert 10 * sharp >= 9 * len(bounds), (sharp, len(bounds))


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_rank_of_the_next_batch(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    src, dst = s.src[E0:E0 + B].copy(), s.dst[E0:E0 + B].copy()
    cand = eng.dst_nodes.cpu().numpy()
    C = cand.size
    assert np.isin(dst, cand).all()
    rank, gt, eq, n, prob, logits = _np(eng.rank(src, dst, return_scores=True))
    assert logits.shape == (B, C) and rank.dtype == np.float64 and gt.dtype == eq.dtype == n.dtype == np.int64
    plain = _np(eng.rank(src, dst))
    assert len(plain) == 5 and all(np.array_equal(x, y) for x, y in zip(plain, (rank, gt, eq, n, prob)))
    # exact on the returned logits: the target's column is its node's
    at = np.array([int(np.flatnonzero(cand == x)[0]) for x in dst])
    full = np.concatenate([logits, logits[:, at]], axis=1)
    key = np.concatenate([cand, dst])
    wgt, weq, wn, wrank = link_rank_ref(full, C, C + np.arange(B), key)
    assert np.array_equal(gt, wgt) and np.array_equal(eq, weq) and np.array_equal(n, wn)
    assert np.array_equal(rank, wrank) and not np.isnan(rank).any()
    assert (n == C - 1).all()                                              # every candidate but the target's own node
    tl = torch.from_numpy(full[np.arange(B), C + np.arange(B)])
    assert float((torch.from_numpy(prob) - torch.sigmoid(tl)).abs().max()) <= 1e-6
    # against the oracle
    want = _oracle_logits(ref, lref, ev_t, ev_msg, src, key).numpy()
    _close(torch.from_numpy(logits), torch.from_numpy(want[:, :C]), TOL)
    bounds, _ = _bounds(want, key, C)
    _check_bracket(gt, eq, n, bounds)
    _close(torch.from_numpy(prob), eng.score(src, dst), TOL)
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_exclude_seen(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    src = _sources(eng, s)                                                 # NS full ring rows, then an empty one
    cand = eng.dst_nodes.cpu().numpy()
    C = cand.size
    nbr, e_id = _ring(eng)
    ptr, keys = seen_lists(nbr, e_id, src)
    assert (np.diff(ptr)[:NS] > 0).all() and ptr[NS + 1] == ptr[NS]
    # destinations chosen on the oracle: the candidate of median logit (seen candidates lie above and below it);
    # row 0's is a node of its own ring row
    base = _oracle_logits(ref, lref, ev_t, ev_msg, src, cand).numpy()
    dst = np.array([cand[np.argsort(base[q])[C // 2]] for q in range(len(src))])
    own = [x for x in keys[ptr[0]:ptr[1]] if x in cand]
    assert own
    dst[0] = own[0]
    key = np.concatenate([cand, dst])
    want = _oracle_logits(ref, lref, ev_t, ev_msg, src, key).numpy()
    rank_u, gt_u, eq_u, n_u, prob_u, lg_u = _np(eng.rank(src, dst, return_scores=True))
    rank_f, gt_f, eq_f, n_f, prob_f, lg_f = _np(eng.rank(src, dst, return_scores=True, exclude_seen=True))
    assert np.array_equal(lg_u, lg_f) and np.array_equal(prob_u, prob_f)  # unmasked, the same bits
    at = np.array([int(np.flatnonzero(cand == x)[0]) for x in dst])
    full = np.concatenate([lg_f, lg_f[:, at]], axis=1)
    wgt, weq, wn, wrank = link_rank_ref(full, C, C + np.arange(len(src)), key, None, ptr, keys)
    assert np.array_equal(gt_f, wgt) and np.array_equal(eq_f, weq) and np.array_equal(n_f, wn)
    assert np.array_equal(rank_f, wrank)
    assert (gt_f <= gt_u).all() and (n_f <= n_u).all()
    assert not np.isnan(rank_f[0]) and n_f[0] == n_u[0] - (len(set(own)) - 1)    # its own node: ranked, not skipped
    assert (rank_f[NS], gt_f[NS], eq_f[NS], n_f[NS]) == (rank_u[NS], gt_u[NS], eq_u[NS], n_u[NS])   # empty ring row
    bounds, m = _bounds(want, key, C, None, ptr, keys)
    _check_bracket(gt_f, eq_f, n_f, bounds, share=False)
    # not vacuous: where the oracle has a seen candidate clearly above the target, the filter lowered gt
    lowered = 0
    for q in range(NS):
        seen = np.isin(cand, keys[ptr[q]:ptr[q + 1]]) & (cand != dst[q])
        if (want[q, :C][seen] > want[q, C + q] + m).any():
            assert gt_f[q] < gt_u[q] and n_f[q] < n_u[q], q
            lowered += 1
    assert lowered > 0
    eng.check()


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_exclude_self_lists_and_outside_destinations(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    src, dst = s.src[E0:E0 + 12].copy(), s.dst[E0:E0 + 12].copy()
    cand = np.arange(N)                                                    # every node: the sources are candidates
    rank, gt, eq, n, prob, lg = _np(eng.rank(src, dst, candidates=cand, return_scores=True))
    rank_s, gt_s, eq_s, n_s, prob_s = _np(eng.rank(src, dst, candidates=cand, exclude_self=True))
    assert (n == N - 1).all() and (n_s == N - 2).all() and np.array_equal(prob, prob_s)
    tl = lg[np.arange(12), dst]
    own = lg[np.arange(12), src]
    assert np.array_equal(gt_s, gt - (own > tl)) and np.array_equal(eq_s, eq - (own == tl))
    # explicit lists: the same exclusion written out, and the destination's own node in a list (it stays ranked)
    lists = [[int(a), int(b)] for a, b in zip(src, dst)]
    got = _np(eng.rank(src, dst, candidates=cand, exclude=lists))
    assert all(np.array_equal(x, y) for x, y in zip(got, (rank_s, gt_s, eq_s, n_s, prob_s)))
    # destinations that are no candidates: ranked against all C of them
    few = np.setdiff1d(np.arange(N), dst)[:90]
    rank_o, gt_o, eq_o, n_o, prob_o, lg_o = _np(eng.rank(src, dst, candidates=few, return_scores=True))
    assert lg_o.shape == (12, 90) and (n_o == 90).all() and not np.isnan(rank_o).any()
    key = np.concatenate([few, dst])
    want = _oracle_logits(ref, lref, ev_t, ev_msg, src, key).numpy()
    bounds, _ = _bounds(want, key, 90)
    _check_bracket(gt_o, eq_o, n_o, bounds, share=False)
    _close(torch.from_numpy(prob_o), eng.score(src, dst), TOL)
    assert np.array_equal(rank_o, 1 + gt_o + 0.5 * eq_o)
    empty = eng.rank([], [])
    assert all(t.numel() == 0 for t in empty)
    with pytest.raises(ValueError):
        eng.rank([1, N], [2, 3])
    with pytest.raises(ValueError):
        eng.rank([1, 2], [2, -1])
    with pytest.raises(ValueError):
        eng.rank([1, 2], [2])
    eng.check()


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_rank_changes_nothing(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    src, dst = s.src[E0:E0 + B].copy(), s.dst[E0:E0 + B].copy()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(eng).items()}
    eng.rank(src, dst)
    eng.rank(src, dst, return_scores=True, exclude_seen=True, exclude_self=True, exclude=[[1, 2]] * B)
    eng.rank(src[:7], dst[:7], candidates=np.arange(40))
    torch.cuda.synchronize()
    after = _state(eng)
    for k, v in before.items():
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]                        # GEN advances by one per embed call
            assert torch.equal(after[k][keep], v[keep]), (k, after[k].tolist(), v.tolist())
            assert int(after[k][3]) > int(v[3]) and int(after[k][11]) == 0
        else:
            assert torch.equal(_bits(after[k]), _bits(v)), k


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_rank_events_is_rank_then_observe(layers, aggr):
    s = _stream()
    sd = _ref(layers, aggr).state_dict()
    negs = _negs(s, B, KN)
    a, b, c = (_engine(s, sd, layers, aggr) for _ in range(3))
    for e in (a, b, c):
        e.flush()
        _eval_batches(e, s, negs, B, 0, 6)
    got = a.rank_events(E0, B, exclude_seen=True)
    want = b.rank(s.src[E0:E0 + B].copy(), s.dst[E0:E0 + B].copy(), exclude_seen=True)
    b.observe(E0, B)
    c.observe(E0, B)
    torch.cuda.synchronize()
    assert len(got) == 5
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(_bits(x) if x.dtype == torch.float32 else x.view(torch.int64),
                                                  _bits(y) if y.dtype == torch.float32 else y.view(torch.int64))
    sa, sb, sc = _state(a), _state(b), _state(c)
    keep = [i for i in range(24) if i != 3]
    for k in sa:
        if k == "ctl":
            assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k][keep], sc[k][keep])
        elif k == "node_gen":
            # the generation stamps of the nodes the batch touched hold the GEN word, which rank()'s embed calls
            # advanced: against the observe-only twin the same nodes are stamped, with its own GEN
            assert torch.equal(sa[k], sb[k])
            ga, gc = int(sa[k].max()), int(sc[k].max())                   # the latest stamp: this batch's
            assert ga > gc and torch.equal(sa[k] == ga, sc[k] == gc)
            assert torch.equal(sa[k][sa[k] != ga], sc[k][sc[k] != gc])
        else:
            assert torch.equal(_bits(sa[k]), _bits(sb[k])) and torch.equal(_bits(sa[k]), _bits(sc[k])), k
    # a partial batch, and observe()'s argument checks
    part = a.rank_events(E0 + B, 7)
    assert part[0].shape == (7,)
    for start, n in ((0, B + 1), (-1, 5), (NEV - 3, 5), (0, -1)):
        with pytest.raises(ValueError):
            a.rank_events(start, n)
    a.world = 2
    try:
        with pytest.raises(ValueError):
            a.rank_events(E0, B)
    finally:
        a.world = 1
    for e in (a, b, c):
        e.check()


def test_dropin_rank_stream_equals_the_hand_loop_on_a_twin():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.data import SplitLoader, TemporalData
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TGNModel
    assert pyg_epoch_utils.rank_stream is tgn_epoch.rank_stream
    s = _stream()
    sd = _ref(1, "last").state_dict()
    data = TemporalData(src=torch.from_numpy(s.src), dst=torch.from_numpy(s.dst), t=torch.from_numpy(s.t),
                        msg=torch.from_numpy(s.msg))
    loader = SplitLoader(data, 0, 4 * B, B, np.zeros(4 * B, dtype=np.int64))
    model = TGNModel(N, NEV, 16, 32, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(sd)
    nl = LastNeighborLoader(N, 10, device=DEV)
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.rank_stream(model, nl, 0, 10, 5)
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train and eng.num_events == NEV
    twin = _engine(s, sd, 1, "last")
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(twin).items():
            if k not in ("grad", "adam_m", "adam_v"):
                v.copy_(_state(eng)[k])
    twin.flush()
    flushes = []
    flush = eng.flush
    eng.flush = lambda *a, **kw: (flushes.append(1), flush(*a, **kw))[1]
    lo, hi = 4 * B, 4 * B + 130                                            # batches of 50, 50 and 30
    got = pyg_epoch_utils.rank_stream(model, nl, lo, hi, B, ks=(1, 3, 10), exclude_seen=True)
    assert not eng._mode_train and len(flushes) == 1
    ranks = torch.cat([twin.rank_events(a, min(B, hi - a), exclude_seen=True)[0] for a in range(lo, hi, B)])
    assert got["rank"].dtype == torch.float64 and got["rank"].shape == (130,) and got["rank"].is_cuda
    assert torch.equal(got["rank"], ranks) and not bool(torch.isnan(ranks).any())
    r = ranks.cpu().numpy()
    assert set(got) == {"mrr", "rank", "hits@1", "hits@3", "hits@10"}
    assert abs(got["mrr"] - float((1.0 / r).mean())) <= 1e-12
    for k in (1, 3, 10):
        assert abs(got[f"hits@{k}"] - float((r <= k).mean())) <= 1e-12
    assert 0.0 < got["mrr"] <= 1.0 and got["hits@1"] <= got["hits@3"] <= got["hits@10"]
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert torch.equal(_bits(_state(eng)[k]), _bits(_state(twin)[k])), k
    more = tgn_epoch.rank_stream(model, nl, hi, hi + 20, B, candidates=np.arange(N), exclude_self=True)
    assert len(flushes) == 1 and more["rank"].shape == (20,)             # no second flush
    assert set(more) == {"mrr", "rank", "hits@1", "hits@10", "hits@50"}
    with pytest.raises(ValueError):
        tgn_epoch.rank_stream(model, nl, 0, NEV + 1, B)
    with pytest.raises(ValueError):
        tgn_epoch.rank_stream(model, nl, 0, 10, B + 1)
    eng.check()
    twin.check()
