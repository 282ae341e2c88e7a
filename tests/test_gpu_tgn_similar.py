"""GPU tests of TgnEngine.similar (nearest neighbours in embedding space; ops.embed_knn over embed() / the embedding
table) and the drop-in pyg_epoch_utils.similar, on the small engine of test_gpu_tgn_query.py (300 nodes, D = 32, six
eval batches on the engine and on the oracle), model forms (1, "last") and (2, "mean").

  oracle         the embeddings of every node from the oracle's eval forward (_oracle_embed), float64 cosine and dot
                 scores (tests/knn_ref.py).  The returned scores match them at 2e-5 in the `_close` metric (the bound
                 embed() and recommend()'s logits are held to against the same oracle); with tol = 2e-5 and scale =
                 max(|ref|, 1) every returned node's reference score is >= the reference's k-th largest of the allowed
                 set - 2 tol scale and the values are within tol scale; the ids are valid, distinct and never the
                 query itself under exclude_self; and they equal knn_ref's selection on the returned scores exactly;
  exclude_seen   against topk_filter_ref.seen_lists of the ring, exactly, on the returned scores;
  exclude / candidates   explicit lists (unsorted, with an id that is no candidate) and an explicit candidate set
                 with a duplicated node and the queries among them; padding when fewer than k remain;
  cached         cached=True equals cached=False within the slack rule after a clean refresh and right after an
                 observe(); it raises without the table;
  read-only      memory, last_update, ring, stores, parameters and every ctl word but GEN bitwise unchanged, and the
                 next eval_batch gives the bits of a twin engine that never called similar;
  drop-in        pyg_epoch_utils.similar flushes train mode and equals the engine call on a hand-flushed twin;
  arguments      ids outside [0, N), k outside [1, 128] and an unknown metric raise ValueError."""
import numpy as np
import pytest
import torch

import knn_ref
from test_gpu_tgn_query import (B, D, DEV, KN, N, NEV, TOL, _bits, _built, _close, _engine, _eval_batches, _negs,
                                _oracle_embed, _ref, _state, _stream)
from topk_filter_ref import seen_lists

pytestmark = pytest.mark.gpu
FORMS = [(1, "last"), (2, "mean")]
K = 8

_ORACLE = {}


def _oracle_z(layers, aggr):
    """float64 oracle embeddings of every node at the state of _built(layers, aggr), computed once."""
    if (layers, aggr) not in _ORACLE:
        s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
        _ORACLE[(layers, aggr)] = _oracle_embed(ref, lref, ev_t, ev_msg, np.arange(N)).double().numpy()
    return _ORACLE[(layers, aggr)]


def _nodes(s, eng):
    """12 query nodes: sources with a full ring row, a node without history, random ones and a duplicate."""
    e_id = eng.loader.e_id.cpu().numpy()
    full = np.flatnonzero((e_id >= 0).all(axis=1))[:4]
    empty = int(np.flatnonzero((e_id < 0).all(axis=1))[0])
    rnd = np.random.default_rng(6).integers(0, N, 6)
    return np.concatenate([full, [empty], rnd, full[:1]]).astype(np.int64)


def _ids_of(pos, cand):
    return np.where(pos >= 0, cand[np.maximum(pos, 0)], -1)


def _slack_check(ids, val, ref, allowed, k, cand=None):
    """ids [Q, k] node ids (or positions into cand) against reference scores ref [Q, C] and the allowed mask [Q, C]."""
    scale = max(float(np.abs(ref).max()), 1.0)
    for q in range(ref.shape[0]):
        left = int(allowed[q].sum())
        kk = min(k, left)
        assert (ids[q, kk:] == -1).all() and np.isneginf(val[q, kk:]).all(), q
        got = ids[q, :kk]
        assert (got >= 0).all() and len(set(got.tolist())) == kk, (q, got)
        if kk == 0:
            continue
        pos = got if cand is None else np.array([np.flatnonzero((cand == g) & allowed[q])[0] for g in got])
        assert allowed[q][pos].all(), (q, got)
        kth = np.sort(ref[q][allowed[q]])[::-1][kk - 1]
        at = ref[q, pos]
        print(f"q {q}: worst shortfall {float((kth - at).max()):.3e} slack {2 * TOL * scale:.3e} "
              f"value err {float(np.abs(val[q, :kk] - at).max()):.3e} bound {TOL * scale:.3e}")
        assert (at >= kth - 2 * TOL * scale).all(), (q, float((kth - at).max()), 2 * TOL * scale)
        assert np.abs(val[q, :kk] - at).max() <= TOL * scale


@pytest.mark.parametrize("metric", knn_ref.METRICS)
@pytest.mark.parametrize("layers,aggr", FORMS)
def test_similar_against_the_oracle(layers, aggr, metric):
    s, eng, *_ = _built(layers, aggr)
    nodes = _nodes(s, eng)
    z = _oracle_z(layers, aggr)
    ref = knn_ref.scores(z[nodes], z, metric)
    score, ids, scores = eng.similar(nodes, K, metric=metric, return_scores=True)
    assert score.shape == ids.shape == (len(nodes), K) and scores.shape == (len(nodes), N)
    assert score.dtype == torch.float32 and ids.dtype == torch.long
    _close(scores, torch.from_numpy(ref), TOL)
    ids_n, val = ids.cpu().numpy(), score.cpu().double().numpy()
    assert (ids_n >= 0).all() and (ids_n < N).all()
    assert (ids_n != nodes[:, None]).all()                                  # never the query itself
    allowed = np.arange(N)[None, :] != nodes[:, None]
    _slack_check(ids_n, val, ref, allowed, K)
    wi, wv = knn_ref.select(scores.cpu().numpy(), K, None, nodes, None, None)
    assert np.array_equal(ids_n, wi) and np.array_equal(score.cpu().numpy(), wv)
    assert torch.equal(ids[0], ids[-1]) and torch.equal(score[0], score[-1])  # the duplicated query: the same row
    # exclude_self=False: under cosine a node is its own nearest neighbour (score 1 within rounding)
    s2, i2 = eng.similar(nodes, 3, metric=metric, exclude_self=False)
    _slack_check(i2.cpu().numpy(), s2.cpu().double().numpy(), ref, np.ones_like(allowed), 3)
    if metric == "cosine":
        assert float((s2[:, 0] - 1).abs().max()) <= 1e-6
        own = ref[np.arange(len(nodes)), i2[:, 0].cpu().numpy()]
        assert (own >= 1 - 2 * TOL).all()
    # without return_scores: the same selection
    s3, i3 = eng.similar(nodes, K, metric=metric)
    assert torch.equal(i3, ids) and torch.equal(s3, score)
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_exclude_seen(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    nodes = _nodes(s, eng)
    ptr, keys = seen_lists(eng.loader.neighbors.cpu().numpy(), eng.loader.e_id.cpu().numpy(), nodes)
    assert (np.diff(ptr)[:4] > 0).all() and ptr[5] == ptr[4]
    score, ids, scores = eng.similar(nodes, K, exclude_seen=True, return_scores=True)
    plain = eng.similar(nodes, K, return_scores=True)
    assert torch.equal(scores, plain[2])                                    # unmasked, and the same bits
    ids_n = ids.cpu().numpy()
    for q in range(len(nodes)):
        assert not np.isin(ids_n[q], keys[ptr[q]:ptr[q + 1]]).any(), q
    wi, wv = knn_ref.select(scores.cpu().numpy(), K, None, nodes, ptr, keys)
    assert np.array_equal(ids_n, wi) and np.array_equal(score.cpu().numpy(), wv)
    assert torch.equal(ids[4], plain[1][4]) and torch.equal(score[4], plain[0][4])   # the empty ring row
    # without exclude_self the query may come back, its ring row still may not
    s2, i2, sc2 = eng.similar(nodes, K, exclude_seen=True, exclude_self=False, metric="dot", return_scores=True)
    wi, wv = knn_ref.select(sc2.cpu().numpy(), K, None, None, ptr, keys)
    assert np.array_equal(i2.cpu().numpy(), wi) and np.array_equal(s2.cpu().numpy(), wv)
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_explicit_exclude_lists_and_candidates(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    nodes = _nodes(s, eng)
    Q = len(nodes)
    z = _oracle_z(layers, aggr)
    rng = np.random.default_rng(12)
    cand = rng.permutation(N)[:90].astype(np.int64)
    cand[:4] = nodes[:4]                                                   # queries among the candidates
    cand[50] = cand[10]                                                    # a duplicated node
    cand[60] = nodes[0]                                                    # and a query twice
    extra = [rng.permutation(N)[:int(n)].tolist() for n in rng.integers(0, 30, Q)]   # unsorted; some are no candidates
    extra[1] = []
    extra[2] = [int(c) for c in cand[5:]]                                  # all but five positions (fewer than K left)
    ptr = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum([len(r) for r in extra], out=ptr[1:])
    keys = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in extra])
    for metric in knn_ref.METRICS:
        score, ids, scores = eng.similar(nodes, K, candidates=cand, metric=metric, exclude=extra, return_scores=True)
        assert scores.shape == (Q, 90)
        ref = knn_ref.scores(z[nodes], z[cand], metric)
        _close(scores, torch.from_numpy(ref), TOL)
        wi, wv = knn_ref.select(scores.cpu().numpy(), K, cand, nodes, ptr, keys)
        assert np.array_equal(ids.cpu().numpy(), _ids_of(wi, cand)) and np.array_equal(score.cpu().numpy(), wv)
        allowed = (cand[None, :] != nodes[:, None]) & np.stack([~np.isin(cand, r) for r in extra])
        assert allowed[2].sum() < K and (ids[2] == -1).any() and bool(torch.isneginf(score[2][ids[2] < 0]).all())
        # positions of a duplicated node tie: compare by position through the reference selection, slack on the rest
        sc = scores.cpu().numpy()
        assert np.array_equal(sc[:, 50], sc[:, 10])
        val = score.cpu().double().numpy()
        scale = max(float(np.abs(ref).max()), 1.0)
        for q in range(Q):
            kk = min(K, int(allowed[q].sum()))
            if kk:
                kth = np.sort(ref[q][allowed[q]])[::-1][kk - 1]
                at = ref[q, wi[q, :kk]]
                assert (at >= kth - 2 * TOL * scale).all() and np.abs(val[q, :kk] - at).max() <= TOL * scale
    # the (ptr, ids) form of exclude gives the same
    got = eng.similar(nodes, K, candidates=cand, exclude=(ptr, np.concatenate([np.asarray(r, dtype=np.int64)
                                                                              for r in extra])))
    want = eng.similar(nodes, K, candidates=cand, exclude=extra)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # more slots than candidates
    s5, i5 = eng.similar(nodes[:3], K, candidates=cand[4:9], exclude_self=False)
    assert bool((i5[:, 5:] == -1).all()) and bool(torch.isneginf(s5[:, 5:]).all())
    assert np.array_equal(np.sort(i5[:, :5].cpu().numpy(), axis=1), np.tile(np.sort(cand[4:9]), (3, 1)))
    eng.check()


def _within_slack(got, base_scores, allowed, k):
    """A selection (score [Q, k], ids [Q, k]) against another call's scores [Q, N] as the reference."""
    _slack_check(got[1].cpu().numpy(), got[0].cpu().double().numpy(), base_scores.cpu().double().numpy(), allowed, k)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_cached_equals_uncached_within_the_slack(layers, aggr):
    s = _stream()
    eng = _engine(s, _ref(layers, aggr).state_dict(), layers, aggr)
    eng.flush()
    negs = _negs(s, B, KN)
    _eval_batches(eng, s, negs, B, 0, 6)
    nodes = _nodes(s, eng)
    allowed = np.arange(N)[None, :] != nodes[:, None]
    with pytest.raises(RuntimeError, match="embedding table"):
        eng.similar(nodes, K, cached=True)
    eng.enable_embedding_table()
    for step in range(2):
        if step == 1:
            eng.observe(6 * B, B)                                          # rows go stale: the refresh re-embeds them
        for metric in knn_ref.METRICS:
            base = eng.similar(nodes, K, metric=metric, return_scores=True)
            got = eng.similar(nodes, K, metric=metric, cached=True, return_scores=True)
            _close(got[2], base[2], TOL)
            _within_slack(got, base[2], allowed, K)
            assert bool((got[1] != torch.from_numpy(nodes).to(DEV)[:, None]).all())
        # explicit candidates: a gather from the table
        cand = np.random.default_rng(3).permutation(N)[:70]
        base = eng.similar(nodes, K, candidates=cand, return_scores=True, exclude_seen=True)
        got = eng.similar(nodes, K, candidates=cand, return_scores=True, exclude_seen=True, cached=True)
        _close(got[2], base[2], TOL)
    # the default candidates read the table itself: the scores are those of its rows
    tab = eng.embedding_table().clone()
    from tgnx import ops
    want = ops.embed_knn(tab[torch.from_numpy(nodes).to(DEV)], tab, K, q_key=torch.from_numpy(nodes).to(DEV))
    got = eng.similar(nodes, K, cached=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_similar_changes_nothing_and_eval_goes_on(layers, aggr):
    s = _stream()
    sd = _ref(layers, aggr).state_dict()
    negs = _negs(s, B, KN)
    a, b = (_engine(s, sd, layers, aggr) for _ in range(2))
    for e in (a, b):
        e.flush()
        _eval_batches(e, s, negs, B, 0, 6)
    nodes = _nodes(s, a)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(a).items()}
    a.similar(nodes, K)
    a.similar(nodes, 5, candidates=np.arange(40), metric="dot", return_scores=True, exclude_self=False)
    a.similar(nodes, K, exclude_seen=True, exclude=[[1, 2]] * len(nodes))
    torch.cuda.synchronize()
    after = _state(a)
    for k, v in before.items():
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]                        # GEN advances by one per embed call
            assert torch.equal(after[k][keep], v[keep]), (k, after[k].tolist(), v.tolist())
            assert int(after[k][3]) > int(v[3]) and int(after[k][11]) == 0
        else:
            assert torch.equal(_bits(after[k]), _bits(v)), k
    ra = _eval_batches(a, s, negs, B, 6, 1)
    a.similar(nodes[:3], 4)
    ra += _eval_batches(a, s, negs, B, 7, 1)
    rb = _eval_batches(b, s, negs, B, 6, 2)
    for (pa, na, qa), (pb, nb, qb) in zip(ra, rb):
        assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(qa, qb)
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert torch.equal(_bits(_state(a)[k]), _bits(_state(b)[k])), k


def test_dropin_similar_equals_the_engine_call_on_a_twin():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.data import SplitLoader, TemporalData
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TGNModel
    s = _stream()
    sd = _ref(1, "last").state_dict()
    data = TemporalData(src=torch.from_numpy(s.src), dst=torch.from_numpy(s.dst), t=torch.from_numpy(s.t),
                        msg=torch.from_numpy(s.msg))
    loader = SplitLoader(data, 0, 4 * B, B, np.zeros(4 * B, dtype=np.int64))
    model = TGNModel(N, NEV, 16, D, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(sd)
    nl = LastNeighborLoader(N, 10, device=DEV)
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.similar(model, nl, [1, 2], 3)
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train
    twin = _engine(s, sd, 1, "last")
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(twin).items():
            if k not in ("grad", "adam_m", "adam_v"):
                v.copy_(_state(eng)[k])
    twin.flush()
    nodes = torch.from_numpy(s.src[150:162].copy())
    want = twin.similar(nodes, 6, exclude_seen=True)
    got = pyg_epoch_utils.similar(model, nl, nodes, 6, exclude_seen=True)
    assert not eng._mode_train                                             # switched to eval: flushed
    assert len(got) == 2 and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    got = tgn_epoch.similar(model, nl, nodes, 4, candidates=np.arange(100), metric="dot", exclude_self=False,
                            exclude=[[3, 4]] * 12)
    want = twin.similar(nodes, 4, candidates=np.arange(100), metric="dot", exclude_self=False, exclude=[[3, 4]] * 12)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    # cached: the table is enabled by the drop-in
    assert eng._emb_tab is None
    got = pyg_epoch_utils.similar(model, nl, nodes, 6, cached=True)
    assert eng._emb_tab is not None
    twin.enable_embedding_table()
    want = twin.similar(nodes, 6, cached=True)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def test_bad_arguments_raise_value_error():
    s, eng, *_ = _built(1, "last")
    for bad in ([N], [-1], [3, N + 5]):
        with pytest.raises(ValueError):
            eng.similar(bad, 3)
        with pytest.raises(ValueError):
            eng.similar([1, 2], 3, candidates=bad)
    with pytest.raises(ValueError):
        eng.similar([1, 2], 3, exclude=[[N], []])
    with pytest.raises(ValueError):
        eng.similar([N], 3, exclude_seen=True)                             # refused before the ring row is read
    for k in (0, -1, 129):
        with pytest.raises(ValueError):
            eng.similar([1, 2], k)
    with pytest.raises(ValueError):
        eng.similar([1, 2], 3, metric="euclidean")
    assert eng.similar([], 3)[0].shape == (0, 3)
    eng.check()
