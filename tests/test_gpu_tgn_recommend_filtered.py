"""GPU tests of TgnEngine.recommend_filtered / score and the drop-in tgn_epoch.recommend_filtered.

Setup: that of test_gpu_tgn_query.py (its helpers and its built engines are shared): a 600-event wiki-shaped stream
over 300 nodes, msg_dim 16, D = 32, ring 10, parameters from a RefTGN state dict, 6 eval batches on engine and oracle;
layers in {1, 2} x aggr in {last, mean}.

  exclude_seen   sources with full rings, k = 20: no returned id is among the source's valid ring entries; the result
                 equals topk_filter_ref.filtered_topk on the logits the same call returns, exactly; those logits match
                 the oracle's all-pairs logits at 2e-5 (`_close`); and the filter does something: at least one source
                 loses a candidate from its unfiltered list (checked on the oracle's CPU logits when this was written:
                 in each of the four forms at least four of the five sources have a seen candidate whose logit lies
                 above the unfiltered 21st by 0.027 .. 0.109, against 2 tol scale = 4e-5, so it is in the unfiltered
                 top 20 whatever the rounding); a source with an empty ring row gets the unfiltered answer;
  exclude_self, exclude as lists of lists (merged with the seen rows);
  per_source     exact against the returned ragged logits, the logits against the oracle's pair logits at 2e-5, ids
                 inside each source's list, an empty list all padding; combined with exclude_seen / exclude_self;
  score          against the oracle's link_pred on its eval-forward embeddings at 2e-5;
  read-only      memory, last_update, stores, ring, parameters, moments and every ctl word but GEN bit-identical after
                 all of the above;
  drop-in        tgn_epoch.recommend_filtered(..., exclude_seen=True) equals the engine call on a twin."""
import numpy as np
import pytest
import torch

from test_gpu_tgn_query import (B, DEV, FORMS, KN, N, NEV, TOL, _bits, _built, _close, _engine, _oracle_embed, _ref,
                                _state, _stream)
from topk_filter_ref import filtered_topk, lists_topk, seen_lists

pytestmark = pytest.mark.gpu
K = 20
NS = 5


def _ring(eng):
    return eng.loader.neighbors.cpu().numpy(), eng.loader.e_id.cpu().numpy()


def _sources(eng, s):
    """The NS source nodes of the stream whose ring rows are full (all 10 entries valid) and one node without
    history."""
    nbr, e_id = _ring(eng)
    full = np.flatnonzero((e_id >= 0).all(axis=1))
    full = full[np.isin(full, s.src[:6 * B])][:NS]
    assert full.size == NS
    empty = int(np.flatnonzero((e_id < 0).all(axis=1))[0])
    return np.concatenate([full, [empty]]).astype(np.int64)


def _oracle_logits(ref, lref, ev_t, ev_msg, src, cand):
    z = _oracle_embed(ref, lref, ev_t, ev_msg, np.concatenate([src, cand]))
    lp = ref.link_pred
    with torch.no_grad():
        return lp.lin_final((lp.lin_src(z[:len(src)])[:, None] + lp.lin_dst(z[len(src):])[None]).relu()).squeeze(-1)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_exclude_seen(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    src = _sources(eng, s)
    cand = eng.dst_nodes.cpu().numpy()
    nbr, e_id = _ring(eng)
    val, ids, logits = eng.recommend_filtered(src, K, return_scores=True, exclude_seen=True)
    uval, uids, ulogits = eng.recommend(src, K, return_scores=True)
    assert torch.equal(logits, ulogits)                                    # unmasked, and the same bits
    _close(logits, _oracle_logits(ref, lref, ev_t, ev_msg, src, cand), TOL)
    ptr, keys = seen_lists(nbr, e_id, src)
    assert (np.diff(ptr)[:NS] > 0).all() and ptr[NS + 1] == ptr[NS]
    ids_n, lg = ids.cpu().numpy(), logits.cpu().numpy()
    for q in range(len(src)):
        assert not np.isin(ids_n[q], keys[ptr[q]:ptr[q + 1]]).any(), q
    wi, wv = filtered_topk(lg, cand, None, ptr, keys, K)
    assert np.array_equal(ids_n, np.where(wi >= 0, cand[np.maximum(wi, 0)], -1))
    pad = wi < 0
    assert float((val.cpu() - torch.sigmoid(torch.from_numpy(wv))).abs()[torch.from_numpy(~pad)].max()) <= 1e-6
    # not vacuous: the filter removed something the unfiltered call recommends
    changed = [q for q in range(NS) if not torch.equal(ids[q], uids[q])]
    assert changed, "no source's recommendation changed"
    assert torch.equal(ids[NS], uids[NS]) and torch.equal(val[NS], uval[NS])   # the empty ring row: nothing to exclude
    eng.check()


def test_stale_ring_words_are_not_exclusions():
    """reset_state leaves the ring's node words in place and invalidates e_id: nothing is 'seen' afterwards."""
    s = _stream()
    eng = _engine(s, _ref(1, "last").state_dict(), 1, "last")
    eng.flush()
    for st in range(2):
        eng.eval_batch(st * B, B, torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(B, KN))))
    src = torch.from_numpy(s.src[:6].copy())
    eng.reset_state()
    nbr, e_id = _ring(eng)
    assert (e_id[src.numpy()] < 0).all()
    got = eng.recommend_filtered(src, 5, exclude_seen=True)
    want = eng.recommend(src, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if (nbr[src.numpy()] >= 0).any():                                      # stale ids present: they would have hit
        stale = np.unique(nbr[src.numpy()][nbr[src.numpy()] >= 0])
        assert np.isin(stale, s.dst_nodes).any()


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_exclude_self_and_explicit_lists(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    src = _sources(eng, s)
    cand = np.concatenate([src[:5], eng.dst_nodes.cpu().numpy(), src[:2]])          # sources among the candidates
    val, ids, logits = eng.recommend_filtered(src, K, candidates=cand, return_scores=True, exclude_self=True)
    lg = logits.cpu().numpy()
    wi, _ = filtered_topk(lg, cand, src, None, None, K)
    assert np.array_equal(ids.cpu().numpy(), np.where(wi >= 0, cand[np.maximum(wi, 0)], -1))
    assert not (ids.cpu().numpy() == src[:, None]).any()
    # lists of lists, alone and merged with the seen rows
    extra = [[int(c) for c in cand[5 + q:5 + q + 3]] + [int(cand[0])] for q in range(len(src))]
    extra[4] = []
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in extra])])
    keys = np.concatenate([np.sort(e) for e in extra if e]).astype(np.int64)
    v2, i2, l2 = eng.recommend_filtered(src, K, candidates=cand, return_scores=True, exclude=extra)
    assert torch.equal(l2, logits)
    wi, _ = filtered_topk(lg, cand, None, ptr, keys, K)
    assert np.array_equal(i2.cpu().numpy(), np.where(wi >= 0, cand[np.maximum(wi, 0)], -1))
    v3, i3 = eng.recommend_filtered(src, K, candidates=cand, exclude=(ptr, keys), exclude_seen=True, exclude_self=True)
    sptr, skeys = seen_lists(*_ring(eng), src)
    both = [np.sort(np.concatenate([keys[ptr[q]:ptr[q + 1]], skeys[sptr[q]:sptr[q + 1]]])) for q in range(len(src))]
    bptr = np.concatenate([[0], np.cumsum([b.size for b in both])])
    wi, _ = filtered_topk(lg, cand, src, bptr, np.concatenate(both), K)
    assert np.array_equal(i3.cpu().numpy(), np.where(wi >= 0, cand[np.maximum(wi, 0)], -1))
    with pytest.raises(ValueError):
        eng.recommend_filtered(src, 3, exclude=[[N]] * len(src))
    with pytest.raises(ValueError):
        eng.recommend_filtered(src, 3, exclude=extra[:2])
    with pytest.raises(ValueError):
        eng.recommend_filtered([N], 3, exclude_self=True)
    eng.check()


def _per_source_lists(eng, src):
    """Per source a shuffled list of destination nodes with a duplicate; it contains the source's seen nodes; one
    empty list."""
    rng = np.random.default_rng(6)
    dst = eng.dst_nodes.cpu().numpy()
    sptr, skeys = seen_lists(*_ring(eng), src)
    rows = []
    for q in range(len(src)):
        r = np.concatenate([rng.choice(dst, 12 + q, replace=False), skeys[sptr[q]:sptr[q + 1]], [src[q]]])
        r = rng.permutation(r)
        rows.append(np.concatenate([r, r[:1]]).astype(np.int64))
    rows[3] = np.zeros(0, dtype=np.int64)
    return rows


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_per_source(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    src = _sources(eng, s)
    rows = _per_source_lists(eng, src)
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    flat = np.concatenate(rows)
    seg = np.repeat(np.arange(len(src)), np.diff(ptr))
    val, ids, logits = eng.recommend_filtered(src, 7, return_scores=True, per_source=rows)
    assert val.shape == ids.shape == (len(src), 7) and logits.shape == (flat.size,)
    lg, ids_n = logits.cpu().numpy(), ids.cpu().numpy()
    assert not np.isnan(lg).any()
    slot, wv = lists_topk(lg, ptr, 7)
    want = np.where(slot >= 0, flat[np.minimum(ptr[:-1, None] + np.maximum(slot, 0), flat.size - 1)], -1)
    assert np.array_equal(ids_n, want)
    assert float((val.cpu() - torch.sigmoid(torch.from_numpy(wv)))[torch.from_numpy(slot >= 0)].abs().max()) <= 1e-6
    assert (ids_n[3] == -1).all() and bool((val[3] == 0).all())            # the empty list: all padding
    for q in range(len(src)):
        assert np.isin(ids_n[q][ids_n[q] >= 0], rows[q]).all()
    # the oracle's logits of exactly these pairs
    z = _oracle_embed(ref, lref, ev_t, ev_msg, np.concatenate([src, flat]))
    lp = ref.link_pred
    with torch.no_grad():
        pair = lp.lin_final((lp.lin_src(z[:len(src)][seg]) + lp.lin_dst(z[len(src):])).relu()).view(-1)
    _close(logits, pair, TOL)
    # the (ptr, ids) form is the same call
    v2, i2 = eng.recommend_filtered(src, 7, per_source=(ptr, flat))
    assert torch.equal(v2, val) and torch.equal(i2, ids)
    # with exclusions: the masked entries are NaN in the returned logits, the rest keep their bits
    v3, i3, l3 = eng.recommend_filtered(src, 7, return_scores=True, per_source=rows, exclude_seen=True,
                                        exclude_self=True)
    sptr, skeys = seen_lists(*_ring(eng), src)
    gone = np.array([flat[e] == src[seg[e]] or flat[e] in skeys[sptr[seg[e]]:sptr[seg[e] + 1]]
                     for e in range(flat.size)])
    assert gone.sum() >= NS * 5
    l3n = l3.cpu().numpy()
    assert np.isnan(l3n[gone]).all() and np.array_equal(l3n[~gone], lg[~gone])
    slot, _ = lists_topk(l3n, ptr, 7)
    want = np.where(slot >= 0, flat[np.minimum(ptr[:-1, None] + np.maximum(slot, 0), flat.size - 1)], -1)
    assert np.array_equal(i3.cpu().numpy(), want)
    with pytest.raises(ValueError):
        eng.recommend_filtered(src, 3, per_source=rows, candidates=[1, 2])
    with pytest.raises(ValueError):
        eng.recommend_filtered(src, 3, per_source=[[N]] * len(src))
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_score_matches_the_oracle(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, N, 40), rng.integers(0, N, 40)
    dst[:3] = src[:3]
    p = eng.score(src, dst)
    assert p.shape == (40,)
    z = _oracle_embed(ref, lref, ev_t, ev_msg, np.concatenate([src, dst]))
    with torch.no_grad():
        want = ref.link_pred(z[:40], z[40:]).view(-1)                     # (returns the sigmoid)
    _close(p, want, TOL)
    assert eng.score([], []).shape == (0,)
    with pytest.raises(ValueError):
        eng.score([1, 2], [3])
    eng.check()


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_filtered_queries_change_nothing(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    src = _sources(eng, s)
    rows = _per_source_lists(eng, src)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(eng).items()}
    eng.recommend_filtered(src, K, exclude_seen=True, exclude_self=True, exclude=[[1, 2]] * len(src))
    eng.recommend_filtered(src, 5, candidates=np.arange(40), return_scores=True, exclude_self=True)
    eng.recommend_filtered(src, 5, per_source=rows, exclude_seen=True, return_scores=True)
    eng.score(src, src[::-1].copy())
    torch.cuda.synchronize()
    after = _state(eng)
    for k, v in before.items():
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]                        # GEN advances by one per embed call
            assert torch.equal(after[k][keep], v[keep]), (k, after[k].tolist(), v.tolist())
            assert int(after[k][3]) > int(v[3]) and int(after[k][11]) == 0
        else:
            assert torch.equal(_bits(after[k]), _bits(v)), k


def test_dropin_recommend_filtered_equals_the_engine_call_on_a_twin():
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
    model = TGNModel(N, NEV, 16, 32, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(sd)
    nl = LastNeighborLoader(N, 10, device=DEV)
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.recommend_filtered(model, nl, [1, 2], 3, exclude_seen=True)
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
    src = torch.from_numpy(s.src[150:162].copy())
    want = twin.recommend_filtered(src, 6, exclude_seen=True)
    got = pyg_epoch_utils.recommend_filtered(model, nl, src, 6, exclude_seen=True)
    assert not eng._mode_train                                             # switched to eval: flushed
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    rows = [[int(x) for x in s.dst_nodes[q:q + 9]] for q in range(12)]
    got = tgn_epoch.recommend_filtered(model, nl, src, 4, per_source=rows, exclude_self=True)
    want = twin.recommend_filtered(src, 4, per_source=rows, exclude_self=True)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
