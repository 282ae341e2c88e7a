"""GPU tests of the embedding table: tgnx_embtab_touch / expand / list, tgnx_tgn_embed_into and the
engine's enable_embedding_table / refresh_embeddings / embedding_table / cached queries.

Setup: that of tests/test_gpu_tgn_query.py — a 600-event wiki-shaped stream over 300 nodes (msg_dim 16, D = 32, ring
10), parameters from a RefTGN state dict, dropout 0, six EVAL batches on the engine and on the oracle — over layers in
{1, 2} x aggr in {last, mean}.  Every later batch is taken into the oracle with embtab_ref.oracle_observe.  The stale
ids are compared, exactly, with embtab_ref.stale_ids on the engine's own ring tensors and the batch endpoints; rows
are compared with oracle_embed(arange(N)) at 2e-5 in the `_close` metric, the bound test_gpu_tgn_query.py holds embed
to.  tests/test_embtab_cpu.py shows on the oracle that a touched node moves by more than 100 x that bound, so a row
left stale fails the comparison.

  parity         enable after the six batches: the first refresh returns arange(N), the table meets the oracle;
  increment      observe(50) -> the ids are the reference's, fewer than N, on both sides of node 256 (two workgroups of
                 the list kernels); rows outside keep their bits; the table meets the oracle; a second refresh is empty
                 and changes no bit;
  accumulate     three observes of 8 with no query in between, one refresh;
  eval_batch     marks like observe (five negatives: they are not endpoints);
  edge shapes    B = 1; one repeated pair; a node with an empty ring row touched for the first time; N = 257 with node
                 256 stale (a one-node workgroup); a stale list beyond embed_capacity() = 24 (the chunked path);
  invalidation   flush, reset_state, a train batch, load_stream_state, model.load_state_dict: arange(N) again, the table
                 against the oracle twin (load_stream_state) or against embed(arange(N)) at 4e-5 (two 2e-5 bounds);
  compaction     stales nothing; an observe in the new numbering marks as before;
  growth         grow_nodes(N + 37): old rows keep their bits, exactly the 37 new ids; observe_events(grow=True);
  queries        recommend_cached / recommend_filtered(cached=True) / score_cached / rank(cached=True) /
                 rank_stream(cached=True);
  C calls alone  tgnx_embtab_touch + tgnx_embtab_list on hand-made planes: N = 1, 64, 255, 256, 257 and 262,147 (more
                 than 1024 workgroups: the count scan carries across its rounds), against numpy;
  read-only      off by default (a twin's state is torch.equal, cached=True raises); enabled, everything but the
                 table, the planes and ctl GEN equals a twin without it; world > 1 refused."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from embtab_ref import oracle_observe, stale_ids
from link_rank_ref import link_rank_ref
from test_gpu_tgn_query import _bits, _close, _eval_batches, _stable_topk_ids, _state
from tgn_oracle_steps import oracle_embed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, d, D, B, KN, NEV = 300, 16, 32, 50, 5, 600
TOL = 2e-5
FORMS = [(1, "last"), (1, "mean"), (2, "last"), (2, "mean")]


# ------------------------------------------------------------------ the rig: an engine and its oracle twin
def _first_unseen(s, events, n):
    return int(np.setdiff1d(np.arange(n), np.concatenate([s.src[:events], s.dst[:events]]))[0])


def _edit_pair(s, n, e0):
    s.src[e0:e0 + 4], s.dst[e0:e0 + 4] = s.src[e0], s.dst[e0]


def _edit_first_seen(s, n, e0):
    s.src[e0] = _first_unseen(s, e0 + 1, n)


def _edit_last_node(s, n, e0):
    s.dst[e0] = n - 1


EDITS = {None: None, "pair": _edit_pair, "first_seen": _edit_first_seen, "last_node": _edit_last_node}
_ORACLES = {}


class Rig:
    pass


def _stream(n, batch, edit):
    from tgnx.synth import make_stream
    s = make_stream("tgbl-wiki", seed=5, num_events=NEV, num_nodes=n, msg_dim=d)
    if EDITS[edit] is not None:            # (rows after the six evaluated batches only)
        s.src, s.dst = s.src.copy(), s.dst.copy()
        EDITS[edit](s, n, 6 * batch)
    return s


def _engine(s, sd, layers, aggr, n=N, batch=B, kn=KN, dst_nodes=True):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    model = TGNModel(n, s.num_events, d, D, DEV, ring=10, max_batch=batch, max_neg=kn, aggr=aggr, dropout=0.0,
                     layers=layers)
    model.load_reference_state(sd)
    eng = TgnEngine(model, LastNeighborLoader(n, 10, device=DEV),
                    dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), TgnAdam(model, 1e-3),
                    dst_nodes=s.dst_nodes if dst_nodes else None, seed=7)
    eng.reset_state()
    eng.flush()     # the oracle's first eval() is TGNMemory.train(False): every node's row through the updater once
    return eng


def _oracle(layers, aggr, n, batch, kn, edit):
    """(stream, RefTGN, its loader, ev_t, ev_msg, negatives) after six eval batches; computed once, copied out."""
    key = (layers, aggr, n, batch, kn, edit)
    if key not in _ORACLES:
        from oracle.sampler_ref import RefLastNeighborLoader
        from oracle.tgn_ref import RefTGN, eval_step
        s = _stream(n, batch, edit)
        torch.manual_seed(0)
        ref = RefTGN(n, d, hidden=D, aggr=aggr, dropout=0.0, layers=layers)
        sd = copy.deepcopy(ref.state_dict())
        negs = torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(8 * batch, kn)))
        lref = RefLastNeighborLoader(n, 10)
        ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
        src, dst = torch.from_numpy(s.src), torch.from_numpy(s.dst)
        for st in range(6):
            sl = slice(st * batch, (st + 1) * batch)
            eval_step(ref, lref, ev_t, ev_msg, src[sl], dst[sl], negs[sl], ev_t[sl], ev_msg[sl])
        _ORACLES[key] = (s, ref, lref, ev_t, ev_msg, negs, sd)
    s, ref, lref, ev_t, ev_msg, negs, sd = _ORACLES[key]
    return s, copy.deepcopy(ref), copy.deepcopy(lref), ev_t, ev_msg, negs, sd


def _rig(layers, aggr, n=N, batch=B, kn=KN, edit=None, dst_nodes=True, enable=True):
    r = Rig()
    r.s, r.ref, r.lref, r.ev_t, r.ev_msg, r.negs, r.sd = _oracle(layers, aggr, n, batch, kn, edit)
    r.n, r.batch, r.layers, r.e0 = n, batch, layers, 6 * batch
    r.eng = _engine(r.s, r.sd, layers, aggr, n, batch, kn, dst_nodes)
    _eval_batches(r.eng, r.s, r.negs, batch, 0, 6)
    if enable:
        r.eng.enable_embedding_table()
    return r


def _oracle_all(r):
    return oracle_embed(r.ref, r.lref, r.ev_t, r.ev_msg, np.arange(r.n))


def _ends(s, lo, hi):
    return np.concatenate([s.src[lo:hi], s.dst[lo:hi]])


def _want_ids(eng, touched):
    ld = eng.loader
    return stale_ids(ld.neighbors.cpu().numpy(), ld.e_id.cpu().numpy(), touched, int(eng.cfg.layers))


def _observe_both(r, lo, hi):
    r.eng.observe(lo, hi - lo)
    oracle_observe(r.ref, r.lref, r.s, r.ev_t, r.ev_msg, lo, hi)


def _check_refresh(r, touched, extra=()):
    """One refresh: the ids are the reference's (plus `extra`), rows outside keep their bits, the table meets the
    oracle.  Returns the ids."""
    eng = r.eng
    before = eng._emb_tab[:r.n].clone()
    ids = eng.refresh_embeddings()
    assert ids.dtype == torch.int64 and ids.is_cuda
    want = np.union1d(_want_ids(eng, touched), np.asarray(extra, dtype=np.int64))
    got = ids.cpu().numpy()
    print(f"stale {got.size} of {r.n} (touched {np.unique(touched).size})")
    assert np.array_equal(got, want), (got, want)
    tab = eng.embedding_table()
    keep = np.setdiff1d(np.arange(r.n), want)
    assert torch.equal(_bits(tab[keep]), _bits(before[keep]))
    _close(tab, _oracle_all(r), TOL)
    eng.check()
    return got


# ------------------------------------------------------------------ parity, increment, accumulation
@pytest.mark.parametrize("layers,aggr", FORMS)
def test_parity_after_enable(layers, aggr):
    r = _rig(layers, aggr)
    ids = r.eng.refresh_embeddings()
    assert torch.equal(ids, torch.arange(N, device=DEV))
    tab = r.eng.embedding_table()
    assert tab.shape == (N, D) and tab.dtype == torch.float32
    _close(tab, _oracle_all(r), TOL)
    assert r.eng.refresh_embeddings().numel() == 0
    r.eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_increment(layers, aggr):
    r = _rig(layers, aggr)
    eng = r.eng
    eng.embedding_table()
    _observe_both(r, r.e0, r.e0 + B)
    got = _check_refresh(r, _ends(r.s, r.e0, r.e0 + B))
    assert 0 < got.size < N
    assert got.min() < 256 <= got.max()                 # the list crosses a workgroup boundary of its kernels
    bits = eng._emb_tab.clone()
    gen = int(eng.ctl[3])
    again = eng.refresh_embeddings()
    assert again.numel() == 0 and again.dtype == torch.int64
    assert torch.equal(_bits(eng._emb_tab), _bits(bits)) and int(eng.ctl[3]) == gen   # no embed launch


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_several_batches_accumulate(layers, aggr):
    r = _rig(layers, aggr)
    r.eng.embedding_table()
    for a in range(r.e0, r.e0 + 24, 8):
        _observe_both(r, a, a + 8)
    got = _check_refresh(r, _ends(r.s, r.e0, r.e0 + 24))
    assert got.size < N


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_eval_batch_marks_like_observe(layers, aggr):
    from oracle.tgn_ref import eval_step
    r = _rig(layers, aggr)
    r.eng.embedding_table()
    sl = slice(r.e0, r.e0 + B)
    r.eng.eval_batch(r.e0, B, r.negs[sl])
    src, dst = torch.from_numpy(r.s.src[sl]), torch.from_numpy(r.s.dst[sl])
    eval_step(r.ref, r.lref, r.ev_t, r.ev_msg, src, dst, r.negs[sl], r.ev_t[sl], r.ev_msg[sl])
    got = _check_refresh(r, _ends(r.s, r.e0, r.e0 + B))
    assert got.size < N


# ------------------------------------------------------------------ the smallest edge shapes
@pytest.mark.parametrize("layers,aggr", FORMS)
@pytest.mark.parametrize("case", ["b1", "pair", "first_seen"])
def test_edge_batches(case, layers, aggr):
    r = _rig(layers, aggr, edit=None if case == "b1" else case)
    eng, s, e0 = r.eng, r.s, r.e0
    eng.embedding_table()
    nb = 4 if case == "pair" else 1
    if case == "pair":
        assert len(set(s.src[e0:e0 + 4])) == 1 and len(set(s.dst[e0:e0 + 4])) == 1
    if case == "first_seen":
        v = int(s.src[e0])
        assert int((eng.loader.e_id[v] >= 0).sum()) == 0 and int((eng.loader.neighbors == v).sum()) == 0
    _observe_both(r, e0, e0 + nb)
    got = _check_refresh(r, _ends(s, e0, e0 + nb))
    assert {int(s.src[e0]), int(s.dst[e0])} <= set(got.tolist()) and got.size < N


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_257_nodes_and_a_one_node_workgroup(layers, aggr):
    n = 257
    r = _rig(layers, aggr, n=n, edit="last_node")
    ids = r.eng.refresh_embeddings()
    assert torch.equal(ids, torch.arange(n, device=DEV))
    _close(r.eng.embedding_table(), _oracle_all(r), TOL)
    _observe_both(r, r.e0, r.e0 + B)
    got = _check_refresh(r, _ends(r.s, r.e0, r.e0 + B))
    assert got[-1] == 256 and got[0] < 256 and got.size < n


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_a_stale_list_beyond_the_embed_capacity(layers, aggr):
    r = _rig(layers, aggr, batch=8, kn=1)
    eng = r.eng
    assert eng.embed_capacity() == 24
    gen = int(eng.ctl[3])
    assert torch.equal(eng.refresh_embeddings(), torch.arange(N, device=DEV))
    assert int(eng.ctl[3]) - gen == -(-N // 24)                              # 13 chunks
    _close(eng.embedding_table(), _oracle_all(r), TOL)
    for a in range(r.e0, r.e0 + 24, 8):
        _observe_both(r, a, a + 8)
    gen = int(eng.ctl[3])
    got = _check_refresh(r, _ends(r.s, r.e0, r.e0 + 24))
    assert 24 < got.size < N and int(eng.ctl[3]) - gen == -(-got.size // 24)


# ------------------------------------------------------------------ what makes everything stale, and what does not
@pytest.mark.parametrize("layers,aggr", FORMS)
@pytest.mark.parametrize("what", ["flush", "reset_state", "train_batch", "load_stream_state", "load_state_dict"])
def test_invalidation(what, layers, aggr):
    r = _rig(layers, aggr)
    eng = r.eng
    eng.embedding_table()
    twin = None
    if what == "load_stream_state":
        saved = eng.stream_state()
        twin = (copy.deepcopy(r.ref), copy.deepcopy(r.lref))
    _observe_both(r, r.e0, r.e0 + B)
    assert 0 < eng.refresh_embeddings().numel() < N
    old = eng._emb_tab[:N].clone()
    if what == "flush":
        eng.flush()
    elif what == "reset_state":
        eng.reset_state()
    elif what == "train_batch":
        neg = torch.from_numpy(np.random.default_rng(1).choice(r.s.dst_nodes, size=B))
        eng.train_batch(r.e0 + B, B, neg=neg, dropout=False)
    elif what == "load_stream_state":
        eng.load_stream_state(saved)
        r.ref, r.lref = twin
    else:
        sd = {k: v.clone() for k, v in eng.model.state_dict().items()}
        sd["gnn.conv.lin_value.weight"] *= 1.25
        eng.model.load_state_dict(sd)
    ids = eng.refresh_embeddings()
    assert torch.equal(ids, torch.arange(N, device=DEV))
    tab = eng.embedding_table()
    if twin is not None:
        _close(tab, _oracle_all(r), TOL)
    else:
        _close(tab, eng.embed(np.arange(N)), 2 * TOL)
    moved = float((tab - old).abs().max())
    print(f"{what}: rows moved by up to {moved:.3e}")
    assert moved > 100 * TOL                                                # (the table was rewritten, not kept)
    assert eng.refresh_embeddings().numel() == 0
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_invalidate_embeddings(layers, aggr):
    r = _rig(layers, aggr)
    eng = r.eng
    eng.embedding_table()
    with torch.no_grad():
        eng.model.gnn.conv.lin_value.weight.mul_(1.25)                       # a raw write the engine cannot see
    assert eng.refresh_embeddings().numel() == 0
    eng.invalidate_embeddings()
    assert torch.equal(eng.refresh_embeddings(), torch.arange(N, device=DEV))
    _close(eng.embedding_table(), eng.embed(np.arange(N)), 2 * TOL)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_compact_events_stales_nothing(layers, aggr):
    r = _rig(layers, aggr)
    eng = r.eng
    eng.embedding_table()
    _observe_both(r, r.e0, r.e0 + B)
    eng.refresh_embeddings()
    bits = eng._emb_tab.clone()
    kept = eng.compact_events(upto=r.e0 + B)                                 # (the unobserved rows are kept verbatim)
    assert kept.numel() < NEV
    assert eng.refresh_embeddings().numel() == 0
    assert torch.equal(_bits(eng._emb_tab), _bits(bits))
    _close(eng.embedding_table(), _oracle_all(r), TOL)
    # the next batch, in the new numbering
    lo = int((kept == r.e0 + B).nonzero()[0])
    assert torch.equal(kept[lo:lo + B].cpu(), torch.arange(r.e0 + B, r.e0 + 2 * B))
    eng.observe(lo, B)
    oracle_observe(r.ref, r.lref, r.s, r.ev_t, r.ev_msg, r.e0 + B, r.e0 + 2 * B)
    got = _check_refresh(r, _ends(r.s, r.e0 + B, r.e0 + 2 * B))
    assert 0 < got.size < N


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_growth(layers, aggr):
    r = _rig(layers, aggr)
    eng, s = r.eng, r.s
    eng.embedding_table()
    eng.observe(r.e0, 8)                                                    # flags pending across the growth
    old = eng._emb_tab[:N].clone()
    touched = _ends(s, r.e0, r.e0 + 8)
    assert eng.grow_nodes(N + 37) == N + 37
    assert torch.equal(_bits(eng._emb_tab[:N]), _bits(old))                  # old rows keep their bits
    ids = eng.refresh_embeddings().cpu().numpy()
    assert np.array_equal(ids, np.union1d(_want_ids(eng, touched), np.arange(N, N + 37)))
    keep = np.setdiff1d(np.arange(N), ids)
    assert torch.equal(_bits(eng._emb_tab[keep]), _bits(old[keep]))
    tab = eng.embedding_table()
    assert tab.shape == (N + 37, D)
    assert float(tab[N:].abs().max()) > 0                                    # a new node's embedding is not zero
    _close(tab, eng.embed(np.arange(N + 37)), 2 * TOL)
    # nothing pending: the growth alone stales exactly the new rows
    old = tab.clone()
    assert eng.grow_nodes(N + 39) == N + 39
    assert np.array_equal(eng.refresh_embeddings().cpu().numpy(), np.arange(N + 37, N + 39))
    assert torch.equal(_bits(eng._emb_tab[:N + 37]), _bits(old))
    # a first-seen node through observe_events(grow=True)
    new = N + 41
    rng = np.random.default_rng(2)
    src, dst = np.array([new, int(s.src[0])]), np.array([int(s.dst[0]), int(s.dst[1])])
    t = np.array([s.t.max() + 1, s.t.max() + 2], dtype=np.float32)
    eng.observe_events(src, dst, t, rng.standard_normal((2, d)).astype(np.float32), grow=True)
    assert eng.cfg.num_nodes == new + 1
    ids = eng.refresh_embeddings().cpu().numpy()
    want = np.union1d(_want_ids(eng, np.concatenate([src, dst])), np.arange(N + 39, new + 1))
    assert np.array_equal(ids, want) and new in ids
    _close(eng.embedding_table(), eng.embed(np.arange(new + 1)), 2 * TOL)
    eng.check()


# ------------------------------------------------------------------ queries
def _oracle_logits(r, src, cand):
    z = _oracle_all(r)
    lp = r.ref.link_pred
    with torch.no_grad():
        return lp.lin_final((lp.lin_src(z[src])[:, None] + lp.lin_dst(z[cand])[None]).relu()).squeeze(-1)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_cached_queries(layers, aggr):
    r = _rig(layers, aggr, dst_nodes=False)                                  # default candidates: every node, in order
    eng, s = r.eng, r.s
    _observe_both(r, r.e0, r.e0 + B)
    rng = np.random.default_rng(4)
    src = rng.integers(0, N, 7)
    allv = np.arange(N)
    # every node in order: the table itself is the candidate operand
    val, ids, logits = eng.recommend_cached(src, 5, return_scores=True)
    assert val.shape == ids.shape == (7, 5) and logits.shape == (7, N)
    _close(logits, _oracle_logits(r, src, allv), TOL)
    lg = logits.cpu().numpy()
    assert np.array_equal(ids.cpu().numpy(), _stable_topk_ids(lg, allv, 5))
    # explicit candidates (a gather), through recommend_filtered
    cand = rng.permutation(N)[:90]
    v2, i2, l2 = eng.recommend_filtered(src, 5, candidates=cand, return_scores=True, cached=True)
    _close(l2, _oracle_logits(r, src, cand), TOL)
    assert np.array_equal(i2.cpu().numpy(), _stable_topk_ids(l2.cpu().numpy(), cand, 5))
    v3, i3, l3 = eng.recommend_filtered(src, 5, return_scores=True, exclude_self=True, cached=True)
    assert torch.equal(l3, logits) and not bool((i3 == torch.from_numpy(src).to(DEV)[:, None]).any())
    rows = [rng.permutation(N)[:20] for _ in src]
    v4, i4, l4 = eng.recommend_filtered(src, 5, return_scores=True, per_source=rows, cached=True)
    want4 = torch.cat([_oracle_logits(r, src[q:q + 1], rows[q])[0] for q in range(len(src))])
    _close(l4, want4, TOL)
    # embed_cached / score_cached / rank(cached=True) against the uncached calls
    _close(eng.embed_cached(src), eng.embed(src), 2 * TOL)
    es, ed = s.src[r.e0 + B:r.e0 + 2 * B].copy(), s.dst[r.e0 + B:r.e0 + 2 * B].copy()
    _close(eng.score_cached(es, ed), eng.score(es, ed), TOL)
    rank, gt, eq, n, prob, rl = (x.cpu().numpy() for x in eng.rank(es, ed, return_scores=True, cached=True))
    _close(torch.from_numpy(prob), eng.rank(es, ed)[4], TOL)
    _close(torch.from_numpy(prob), eng.score(es, ed), TOL)
    assert rl.shape == (B, N)
    full = np.concatenate([rl, rl[:, ed]], axis=1)                           # column N + q: the target of row q
    wgt, weq, wn, wrank = link_rank_ref(full, N, N + np.arange(B), np.concatenate([allv, ed]))
    assert np.array_equal(gt, wgt) and np.array_equal(eq, weq) and np.array_equal(n, wn)
    assert np.array_equal(rank, wrank)
    with pytest.raises(ValueError):
        eng.recommend_cached([N], 3)
    with pytest.raises(ValueError):
        eng.embed_cached([-1])
    eng.check()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_rank_stream_cached(layers, aggr):
    """rank_stream(cached=True) over every remaining event: its MRR is the mean of its own ranks, and its ranks are
    the uncached twin's wherever the oracle separates the destination's logit from its nearest competitor by more
    than 1e-4 (five times the bound the logits are held to) — at least 90 % of the events."""
    import pyg_epoch_utils
    a = _rig(layers, aggr, enable=False)
    b = _rig(layers, aggr, enable=False)
    for r in (a, b):                         # the drop-in finds the engine on the model
        r.eng.model._tgnx_engine = r.eng
        r.eng._mode_train = False
    lo, hi = a.e0, NEV
    cand = np.asarray(a.s.dst_nodes)
    sharp = []
    for st in range(lo, hi, B):              # the oracle's margins, batch by batch at the state before the batch
        src, dst = a.s.src[st:st + B], a.s.dst[st:st + B]
        lg = _oracle_logits(a, src, cand).numpy()
        tl = np.diagonal(_oracle_logits(a, src, dst).numpy())
        for q in range(B):
            sharp.append(np.abs(lg[q][cand != dst[q]] - tl[q]).min() > 1e-4)
        oracle_observe(a.ref, a.lref, a.s, a.ev_t, a.ev_msg, st, st + B)
    sharp = np.array(sharp)
    print(f"events with a margin above 1e-4: {int(sharp.sum())} of {sharp.size}")
    assert 10 * int(sharp.sum()) >= 9 * sharp.size
    got = pyg_epoch_utils.rank_stream(a.eng.model, a.eng.loader, lo, hi, B, cached=True)
    assert a.eng._emb_tab is not None                                        # enabled by the call
    want = pyg_epoch_utils.rank_stream(b.eng.model, b.eng.loader, lo, hi, B)
    assert b.eng._emb_tab is None
    rc, ru = got["rank"].cpu().numpy(), want["rank"].cpu().numpy()
    assert rc.shape == (hi - lo,) and not np.isnan(rc).any()
    assert abs(got["mrr"] - float((1.0 / rc).mean())) <= 1e-12
    print(f"ranks differing: {int((rc != ru).sum())} (where the margin is sharp: {int((rc != ru)[sharp].sum())})")
    assert np.array_equal(rc[sharp], ru[sharp])
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert torch.equal(_bits(_state(a.eng)[k]), _bits(_state(b.eng)[k])), k
    a.eng.check()


# ------------------------------------------------------------------ read-only, off by default, one device only
def _calls(eng, s, e0, cached):
    eng.observe(e0, B)
    src = s.src[e0 + B:e0 + B + 7].copy()
    if cached:
        eng.recommend_cached(src, 5)
        eng.rank(src, s.dst[e0 + B:e0 + B + 7].copy(), cached=True)
    else:
        eng.recommend(src, 5)
        eng.rank(src, s.dst[e0 + B:e0 + B + 7].copy())
    eng.rank_events(e0 + B, B, cached=cached)
    torch.cuda.synchronize()


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_read_only_and_off_by_default(layers, aggr):
    off, ref_, on = (_rig(layers, aggr, enable=False) for _ in range(3))
    assert off.eng._emb_tab is None
    for what in (lambda e: e.recommend_cached([1], 3), lambda e: e.score_cached([1], [2]), lambda e: e.embed_cached([1]),
                 lambda e: e.rank([1], [2], cached=True), lambda e: e.recommend_filtered([1], 3, cached=True),
                 lambda e: e.refresh_embeddings(), lambda e: e.embedding_table()):
        with pytest.raises(RuntimeError, match="embedding table"):
            what(off.eng)
    # disabled: every word of the state, ctl included, is what an engine that never heard of the table leaves
    _calls(off.eng, off.s, off.e0, False)
    ref_.eng.enable_embedding_table()
    ref_.eng.disable_embedding_table()
    assert ref_.eng._emb_tab is None
    _calls(ref_.eng, ref_.s, ref_.e0, False)
    for k, v in _state(off.eng).items():
        assert torch.equal(_bits(v), _bits(_state(ref_.eng)[k])), k
    # enabled: everything but the table, the planes and ctl GEN
    on.eng.enable_embedding_table()
    _calls(on.eng, on.s, on.e0, True)
    for k, v in _state(on.eng).items():
        w = _state(off.eng)[k]
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]
            assert torch.equal(v[keep], w[keep]), (v.tolist(), w.tolist())
            assert int(v[11]) == 0
        elif k != "node_gen":               # (observe stamps node_gen with GEN, which the refreshes advance)
            assert torch.equal(_bits(v), _bits(w)), k
    on.eng.check()


@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 1024 * 256 + 3])
def test_touch_and_list_on_their_own(n):
    """The C calls without an engine: one node, a full wave, one node short of / exactly / one past a workgroup, and
    more than 1024 workgroups (the scan of the workgroups' counts carries across its rounds).  Flags in all three
    planes; ids outside [0, n) in the touched batch are skipped; the planes come back clear; twice the same list."""
    from tgnx import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    p = ctypes.c_void_p
    st = p(torch.cuda.current_stream().cuda_stream)
    planes = (rng.random((3, n)) < 0.02).astype(np.uint8)
    planes[1, n - 1] = 1                                                     # the last node, by D1 alone
    nb = min(64, 4 * n)
    src = rng.integers(-2, n + 2, nb)
    dst = rng.integers(0, n, nb)
    ends = np.concatenate([src, dst])
    want = np.flatnonzero(planes.any(0) | np.isin(np.arange(n), ends[(ends >= 0) & (ends < n)]))
    ws = torch.empty(int(L.tgnx_embtab_list_ws_bytes(n)), dtype=torch.uint8, device=DEV)
    lists = []
    for _ in range(2):
        flags = torch.from_numpy(planes.reshape(-1).copy()).to(DEV)
        ids = torch.full((n,), -7, dtype=torch.long, device=DEV)
        cnt = torch.full((1,), -1, dtype=torch.long, device=DEV)
        s_d, d_d = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
        assert L.tgnx_embtab_touch(p(s_d.data_ptr()), p(d_d.data_ptr()), nb, n, p(flags.data_ptr()), st) == 0
        assert L.tgnx_embtab_list(p(flags.data_ptr()), n, 2, p(ids.data_ptr()), p(cnt.data_ptr()), p(ws.data_ptr()),
                                  ws.numel(), st) == 0
        torch.cuda.synchronize()
        assert int(cnt) == want.size
        assert np.array_equal(ids[:want.size].cpu().numpy(), want)
        assert bool((ids[want.size:] == -7).all())                           # nothing written past the count
        assert not bool(flags.any())
        lists.append(ids.clone())
    assert torch.equal(lists[0], lists[1])
    # layers = 1 does not read the D2 plane
    flags = torch.zeros(3 * n, dtype=torch.uint8, device=DEV)
    flags[2 * n:] = 1
    flags[0] = 1
    assert L.tgnx_embtab_list(p(flags.data_ptr()), n, 1, p(ids.data_ptr()), p(cnt.data_ptr()), p(ws.data_ptr()),
                              ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert int(cnt) == 1 and int(ids[0]) == 0 and not bool(flags.any())
    assert L.tgnx_embtab_list(p(flags.data_ptr()), n, 3, p(ids.data_ptr()), p(cnt.data_ptr()), p(ws.data_ptr()),
                              ws.numel(), st) == -1                          # TGNX_EINVAL: layers
    assert L.tgnx_embtab_list(p(flags.data_ptr()), n, 1, p(ids.data_ptr()), p(cnt.data_ptr()), p(ws.data_ptr()),
                              0, st) == -1                                   # a workspace too small


def test_world_above_one_is_refused():
    from tgnx import _lib
    r = _rig(1, "last")
    eng = r.eng
    eng.embedding_table()
    L = _lib.lib()
    b = eng._buffers(0)
    xrows = torch.zeros(16, D + 4, device=DEV)
    b.xrows, b.xcap = xrows.data_ptr(), 16                                   # a data-parallel engine's buffers
    ids = torch.arange(4, device=DEV)
    bits = eng._emb_tab.clone()
    gen = int(eng.ctl[3])
    rc = L.tgnx_embtab_expand(ctypes.byref(eng.cfg), ctypes.byref(b), ctypes.c_void_p(eng._emb_flags.data_ptr()),
                              eng._stream())
    assert rc == -1 and b"one device only" in L.tgnx_last_error()            # TGNX_EINVAL
    rc = L.tgnx_tgn_embed_into(ctypes.byref(eng.cfg), ctypes.byref(b), ctypes.c_void_p(ids.data_ptr()), 4,
                               ctypes.c_void_p(eng._emb_tab.data_ptr()), eng._stream())
    assert rc == -1 and b"one device only" in L.tgnx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng._emb_tab), _bits(bits)) and int(eng.ctl[3]) == gen      # nothing was launched
    assert not bool(eng._emb_flags.any())
    eng.world = 2
    try:
        eng.disable_embedding_table()
        with pytest.raises(ValueError, match="one device only"):
            eng.enable_embedding_table()
        with pytest.raises(ValueError):
            eng.observe(r.e0, B)                                             # (as observe refuses it)
    finally:
        eng.world = 1
    eng.check()
