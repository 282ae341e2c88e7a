"""train / test of the PyG TGN memory path (the canonical loop the reference's
pyg_epoch_utils.py:9-147 carries commented out, :106-137) on the fused HIP step (tgnx.tgn.TgnEngine).

  train(model, feats, train_loader, neighbor_loader, neg_dest_sampler, assoc, device, optimizer, criterion)
      -> total_loss = Σ_batches loss·B (pyg_epoch_utils.py:138); prints "ap and auc: ..." (:139-147)
  test(model, feats, loader, neighbor_loader, neg_sampler, assoc, device, optimizer, criterion,
       evaluator, metric, split_mode) -> mean over batches of the batch MRR (epoch_utils.py:163)

Per train epoch: memory.reset_state + neighbor_loader.reset_state (pyg_epoch_utils.py:15-16), then the
bench's step (the parity-set step replayed from captured HIP graphs, TgnEngine.replay_resident); per
batch: negatives from the destination set (NegLinkSamplerDest distribution, drawn on the device),
memory(n_id) with the GRU update of every sampled node, TransformerConv embedding, LinkPredictor,
BCE-with-logits on its sigmoid outputs (as the reference feeds it), update_state, ring insert,
backward, Adam.  test(): the first call after training switches the memory to eval
(TGNMemory.train(False): every node's memory updated from its stored messages, stores cleared,
memory_module.py:209-215); each batch scores [pos, negatives] with the batch-start state, then
updates the stores, the memory and the ring in eval order.

  recommend(model, neighbor_loader, src, k, candidates=None) -> (val [Q, k], node_ids [Q, k]): the k destinations
      the trained model ranks highest for each source at the current stream state (TgnEngine.recommend; read-only)
  recommend_filtered(model, neighbor_loader, src, k, candidates=None, *, exclude_seen, exclude_self, exclude,
      per_source): the same with per-source exclusions or per-source candidate lists (TgnEngine.recommend_filtered)
  similar(model, neighbor_loader, nodes, k, candidates=None, *, metric, exclude_self, exclude_seen, exclude, cached)
      -> (score [Q, k], node_ids [Q, k]): every node's k nearest neighbours in embedding space (TgnEngine.similar)
  explain(model, src, dst, by="slot") -> dict: per pair the logit and, per side, the ring slots the embedding attends
      over with their attention weight and leave-one-out effect on the logit (TgnEngine.explain; 1 hop, read-only);
      explain_recommendations(model, src, k, **filters): recommend_filtered, then explain of the (src, top-k) pairs
  embedding_table(model, neighbor_loader) -> [N, D]: the current embeddings of every node, kept incrementally
      (TgnEngine.embedding_table); recommend_filtered / rank_stream take cached=True to read it
  observe(model, neighbor_loader, src, dst, t, msg, batch=None) -> (start, n): new interactions appended to the event
      table and taken into memory, stores and ring as test() batches would leave them, without negatives or scores
      (TgnEngine.observe_events)
  grow_nodes(model, neighbor_loader, n) -> num_nodes: the node space extended in place for nodes that first appear
      after the model was built (TgnEngine.grow_nodes); observe_grow(...) is observe() that does it from the ids it is given
  compact(model, neighbor_loader, upto=None, capacity=None) -> kept: retire the event-table rows nothing references
      and renumber the rest in order (TgnEngine.compact_events); kept[new] = old
  forget(model, neighbor_loader, ids, compact=False, drop_candidates=False) -> counts: erase nodes from memory, ring
      and stores in place (TgnEngine.forget_nodes)
  tgb_negatives(loader, k, hist_ratio=0.5, ...) -> [hi - lo, k]: TGB's hist_rnd evaluation negatives for a split,
      generated on the device and installed as loader.negatives (tgnx.tgb_negs); edgebank(loader, batch=None) -> the
      MRR of the memorisation baseline EdgeBank-inf under the loader's negatives
  save_stream(model, neighbor_loader, f) / load_stream(model, neighbor_loader, f, optimizer=None, dst_nodes=None):
      the whole stream state (table, memory, stores, ring, ctl; TgnEngine.stream_state) to / from a torch.save file

Reached through pyg_epoch_utils (shim) and through epoch_utils.train / test, which dispatch here for a
{'memory', 'gnn', 'link_pred'} model: the reference script runs with only its model import swapped
(pyg-mem-tgn.py:19 keeps `from epoch_utils import train, test`).

The loaders must be tgnx SplitLoaders (tgnx.data; what utils.getDataWithDependecyBlock returns):
the event table is bound resident in HBM once and batches address it by global row (e_id)."""
from __future__ import annotations

import torch

from .data import SplitLoader
from .tgn import TgnEngine


def _owner(model):
    return model["model"] if isinstance(model, dict) else model


def _engine(model, train_loader, neighbor_loader, optimizer, neg_dest_sampler=None):
    m = _owner(model)
    eng = getattr(m, "_tgnx_engine", None)
    if eng is None or eng.loader is not neighbor_loader:
        if not isinstance(train_loader, SplitLoader):
            raise TypeError("tgnx pyg_epoch_utils needs tgnx.data.SplitLoader batches (the event table is "
                            "bound resident; see utils.getDataWithDependecyBlock)")
        d = train_loader.data
        dst_nodes = getattr(neg_dest_sampler, "dst_nodes", None)
        if dst_nodes is None:
            dst_nodes = torch.unique(torch.as_tensor(d.dst))
        eng = TgnEngine(m, neighbor_loader, dict(src=d.src, dst=d.dst, t=d.t.float(), msg=d.msg.float()),
                        optimizer, dst_nodes=torch.as_tensor(dst_nodes), seed=getattr(neg_dest_sampler, "seed", 0))
        # the per-event train-output log (tgnx_tgn_buffers.out_ev): every replayed step writes its batch's
        # outputs at their event rows, so the epoch's AP / AUC need no copy per step
        eng.out_ev = torch.zeros(eng.cfg.num_events, 2, dtype=torch.float32, device=eng.dev)
        eng.keep_grads = False    # the loop never reads the gradients (Adam fused: TGNX_TGN_NO_GRAD_STORE)
        eng._mode_train = None
        eng._bound = None
        m._tgnx_engine = eng
    return eng


def ap_auc_rows(pos: torch.Tensor, neg: torch.Tensor, chunk_elems: int = 1 << 26):
    """sklearn's average_precision_score / roc_auc_score of each row's labels [1]*P + [0]*N on the scores
    [pos | neg] (pyg_epoch_utils.py:139-143), for a [R, P] / [R, N] pair of score tensors, on their device.
    AUC = the Mann-Whitney statistic with ties counted 1/2 (roc_auc_score's trapezoids); AP = Σ over distinct
    thresholds of Δrecall x precision, i.e. the mean over positives of the precision at the end of their
    tie group (average_precision_score).  Returns float64 [R] tensors (ap, auc)."""
    R, Pn = pos.shape
    Nn = neg.shape[1]
    if R == 0:
        z = torch.zeros(0, dtype=torch.float64, device=pos.device)
        return z, z
    step = max(1, chunk_elems // max(1, Pn * Nn))
    aucs, aps = [], []
    for a in range(0, R, step):
        p, n = pos[a:a + step], neg[a:a + step]
        gt = (p[:, :, None] > n[:, None, :]).sum((1, 2)).double()
        eq = (p[:, :, None] == n[:, None, :]).sum((1, 2)).double()
        aucs.append((gt + 0.5 * eq) / (Pn * Nn))
        sc = torch.cat([p, n], 1)
        y = torch.cat([torch.ones_like(p), torch.zeros_like(n)], 1).double()
        order = torch.argsort(sc, dim=1, descending=True, stable=True)
        ss, yy = sc.gather(1, order), y.gather(1, order)
        tp = yy.cumsum(1)
        asc = (-ss).contiguous()                                   # ascending rows
        end = torch.searchsorted(asc, asc, right=True) - 1         # last position of each tie group
        prec = tp.gather(1, end) / (end + 1).double()
        aps.append((yy * prec).sum(1) / Pn)
    return torch.cat(aps), torch.cat(aucs)


def epoch_ap_auc(out_ev: torch.Tensor, lo: int, hi: int, B: int):
    """Mean over the epoch's batches of the batch AP and AUC (pyg_epoch_utils.py:139-145) from the per-event
    output log: y_pred = sigmoid of the model's sigmoid outputs, as the reference computes it."""
    sc = torch.sigmoid(out_ev[lo:hi])
    n = hi - lo
    full = n // B
    ap, auc = ap_auc_rows(sc[:full * B, 0].view(full, B), sc[:full * B, 1].view(full, B))
    if n > full * B:
        a2, u2 = ap_auc_rows(sc[full * B:, 0].view(1, -1), sc[full * B:, 1].view(1, -1))
        ap, auc = torch.cat([ap, a2]), torch.cat([auc, u2])
    return float(ap.mean()), float(auc.mean())


def train(model, feats, train_loader, neighbor_loader, neg_dest_sampler, assoc, device, optimizer, criterion):
    """One train epoch as the benchmark runs it: the split bound resident, then the parity-set step replayed
    from its captured graphs batch after batch (TgnEngine.replay_resident; the first step of the epoch runs
    eagerly and prefetches the next), negatives drawn on the device, outputs logged per event."""
    eng = _engine(model, train_loader, neighbor_loader, optimizer, neg_dest_sampler)
    B = train_loader.batch_size
    key = (train_loader.lo, train_loader.hi, B)
    if eng._bound != key:
        eng.bind_resident(train_loader.lo, train_loader.hi, B, dropout=True)
        eng._bound = key
        eng._graphs = None
    eng.begin_epoch()                                     # pyg_epoch_utils.py:15-16 (+ the batch cursor)
    eng._mode_train = True
    loss0 = eng.loss_sum()
    if getattr(eng, "_graphs", None) is None:
        eng.capture_resident()
        eng.capture_group(8)                              # (world 1: 8 steps per graph launch)
    eng.replay_resident_n(len(train_loader))
    eng.finish()
    neighbor_loader.cur_e_id = train_loader.hi
    loss = eng.loss_sum() - loss0                         # (synchronises)
    eng.check()
    if train_loader.hi > train_loader.lo:
        ap, auc = epoch_ap_auc(eng.out_ev, train_loader.lo, train_loader.hi, B)
        print("ap and auc: ", ap, auc)
    return loss


@torch.no_grad()
def test(model, feats, loader, neighbor_loader, neg_sampler, assoc, device, optimizer, criterion, evaluator,
         metric, split_mode):
    eng = _engine(model, loader, neighbor_loader, optimizer)
    if eng._mode_train:                                   # TGNMemory.train(False) (memory_module.py:209-215)
        eng.flush()
        eng._mode_train = False
    perf = []
    B = loader.batch_size
    negs_all = loader.negatives
    if (torch.is_tensor(negs_all) and negs_all.dim() == 2 and negs_all.shape[0] == loader.hi - loader.lo
            and loader.hi > loader.lo):
        # a rectangular negatives table: the resident pass (split and negatives bound once, the step replayed from
        # its captured graph, the reciprocal ranks read once at the end); later epochs reuse binding and graphs
        key = getattr(eng, "_eval_bound", None)
        if key is None or key[:3] != (loader.lo, loader.hi, B) or key[3] is not negs_all:
            eng.bind_eval_resident(loader.lo, loader.hi, B, negs_all)
            eng._eval_bound = (loader.lo, loader.hi, B, negs_all)
        if eng._ev_graphs is None:
            eng.capture_eval()
        eng.begin_eval()
        eng.replay_eval_n(len(loader))
        neighbor_loader.cur_e_id = loader.hi
        mrr = eng.eval_mrr()                              # (synchronises)
        eng.check()
        return mrr
    for s in range(loader.lo, loader.hi, B):
        e = min(loader.hi, s + B)
        if negs_all is not None:
            negs = negs_all[s - loader.lo:e - loader.lo]
        else:
            d = loader.data
            rows = neg_sampler.query_batch(d.src[s:e], d.dst[s:e], d.t[s:e], split_mode=split_mode)
            m = min(len(r) for r in rows)                 # epoch_utils.py:48-56
            negs = torch.tensor([list(r)[:m] for r in rows], dtype=torch.long)
        _, _, rr = eng.eval_batch(s, e - s, negs)
        perf.append(rr.clone().mean())
    neighbor_loader.cur_e_id = loader.hi
    torch.cuda.synchronize(eng.dev)
    eng.check()
    return float(torch.stack(perf).mean()) if perf else float("nan")


@torch.no_grad()
def recommend(model, neighbor_loader, src, k, candidates=None):
    """Top-k link recommendation with the engine train() / test() attached to the model: for every node of `src` the
    k candidates (default: the engine's destination set) with the highest LinkPredictor output at the current stream
    state, as (val [Q, k], node_ids [Q, k]).  Read-only (TgnEngine.recommend).  Straight after train() the memory is
    switched to eval first, exactly as test() does (TGNMemory.train(False), memory_module.py:209-215).
    recommend_filtered(..., cached=True) is the form that reads the engine's embedding table."""
    eng = getattr(_owner(model), "_tgnx_engine", None)
    if eng is None or eng.loader is not neighbor_loader:
        raise RuntimeError("tgnx recommend: no engine bound to this model / neighbor_loader yet (run train() or test() "
                           "first: they bind the event table)")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    return eng.recommend(src, k, candidates=candidates)


@torch.no_grad()
def recommend_filtered(model, neighbor_loader, src, k, candidates=None, *, exclude_seen=False, exclude_self=False,
                       exclude=None, per_source=None, cached=False, exclude_history=False, history_since=None):
    """recommend() with per-source exclusions (exclude_seen: the source's recent interaction partners; exclude_self;
    exclude: more node ids per source) or a candidate list per source (per_source), TgnEngine.recommend_filtered's
    keywords passed through.  cached: read the engine's embedding table (enabled here if it is not) instead of
    embedding the sources and candidates again; without exclusions this is recommend() from the table.
    exclude_history / history_since: leave out everything the source has ever met (enable_pair_history() first).
    Read-only; switches the memory to eval first as recommend() does."""
    eng = getattr(_owner(model), "_tgnx_engine", None)
    if eng is None or eng.loader is not neighbor_loader:
        raise RuntimeError("tgnx recommend_filtered: no engine bound to this model / neighbor_loader yet (run train() "
                           "or test() first: they bind the event table)")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    if cached:
        eng.enable_embedding_table()
    return eng.recommend_filtered(src, k, candidates=candidates, exclude_seen=exclude_seen, exclude_self=exclude_self,
                                  exclude=exclude, per_source=per_source, cached=cached,
                                  exclude_history=exclude_history, history_since=history_since)


@torch.no_grad()
def similar(model, neighbor_loader, nodes, k, candidates=None, *, metric="cosine", exclude_self=True, exclude_seen=False,
            exclude=None, cached=False):
    """Nearest neighbours in embedding space with the engine train() / test() attached to the model: for every node of
    `nodes` the k candidates (default: every node) most similar to it at the current stream state, as (score [Q, k],
    node_ids [Q, k]); TgnEngine.similar's keywords passed through (metric "cosine" / "dot"; exclude_self, on by
    default; exclude_seen; exclude).  cached: read the engine's embedding table (enabled here if it is not).
    Read-only; switches the memory to eval first as recommend() does."""
    eng = _bound_engine(model, neighbor_loader, "similar")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    if cached:
        eng.enable_embedding_table()
    return eng.similar(nodes, k, candidates=candidates, metric=metric, exclude_self=exclude_self,
                       exclude_seen=exclude_seen, exclude=exclude, cached=cached)


def _attached_engine(model, what):
    """The engine train() / test() attached to the model (its own neighbor_loader: the calls that take none)."""
    eng = getattr(_owner(model), "_tgnx_engine", None)
    if eng is None:
        raise RuntimeError(f"tgnx {what}: no engine bound to this model yet (run train() or test() first: they bind "
                           "the event table)")
    return eng


@torch.no_grad()
def explain(model, src, dst, by="slot"):
    """Why the model scores the pairs (src[i], dst[i]) as it does, with the engine train() / test() attached to the
    model: TgnEngine.explain's dict — the logit, and per side the ring slots the embedding attended over with their
    attention weight and their leave-one-out effect on the logit (by="slot": one slot removed; by="neighbour": every
    slot of that neighbour).  Read-only; switches the memory to eval first as recommend() does (one flush)."""
    eng = _attached_engine(model, "explain")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    return eng.explain(src, dst, by=by)


@torch.no_grad()
def explain_recommendations(model, src, k, by="slot", **filters):
    """recommend_filtered(src, k, **filters) followed by explain() of the (source, recommended node) pairs.  Returns
    (val [Q, k], node_ids [Q, k], pair [n_pairs, 2] = (row into src, column of node_ids) of every explained pair, the
    explain() dict over those pairs); the -1 padding of node_ids (k beyond the candidate count) is skipped."""
    eng = _attached_engine(model, "explain_recommendations")
    val, ids = recommend_filtered(model, eng.loader, src, k, **filters)[:2]
    pair = (ids >= 0).nonzero()
    return val, ids, pair, eng.explain(eng._ids(src)[pair[:, 0]], ids[pair[:, 0], pair[:, 1]], by=by)


@torch.no_grad()
def rank_stream(model, neighbor_loader, lo, hi, batch, candidates=None, ks=(1, 10, 50), *, exclude_seen=False,
                exclude_self=False, cached=False, exclude_history=False, history_since=None, split_history=False):
    """Prequential full-catalogue ranking over rows [lo, hi) of the event table of the engine train() / test()
    attached to the model: every batch of `batch` events is ranked at the state before it (TgnEngine.rank_events: the
    true destination against every candidate recommend() would choose from, recommend_filtered()'s exclusions), then
    observed.  Returns {"mrr": mean 1 / rank, "hits@k": mean rank <= k for k in ks, "rank": float64 [hi - lo] on the
    device}; skipped events (NaN rank) count as misses.  The means are taken on the device: one synchronisation, at the
    end.  Switches the memory to eval first as recommend() does.  cached: rank from the engine's embedding table
    (enabled here if it is not), so that each batch embeds only the rows the batch before it made stale instead of
    every candidate; ranks may differ from the uncached ones where two competing logits are closer than the
    embeddings' tolerance.
    exclude_history / history_since: TgnEngine.rank's (enable_pair_history() first).  split_history (the same
    requirement): the result also carries "n_repeat" / "n_novel" (a positive is a repeat when the pair history held its
    pair before its batch: one lookup per batch, ahead of the batch's recording), "mrr_repeat" / "mrr_novel" and
    "hits@k_repeat" / "hits@k_novel", the means over each part (numpy's, over the ranks read back; NaN for an empty
    part), and "repeat" (bool [hi - lo] on the device): the number that says whether the model beats memorisation.  The
    other keys are computed exactly as without it."""
    eng = _bound_engine(model, neighbor_loader, "rank_stream")
    lo, hi, batch = int(lo), int(hi), int(batch)
    if not (0 <= lo <= hi <= eng.num_events) or not (0 < batch <= eng.cfg.max_batch):
        raise ValueError(f"rank_stream: rows [{lo}, {hi}) batch {batch} outside the event table ({eng.num_events} "
                         f"events) / max_batch ({eng.cfg.max_batch})")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    if cached:
        eng.enable_embedding_table()
    if split_history:
        eng._pair_set("rank_stream(split_history=True)")
    ranks, reps = [], []
    for a in range(lo, hi, batch):
        b = min(batch, hi - a)
        if split_history:                                    # (the bank as it stood before the batch)
            reps.append(eng.seen(eng.src[a:a + b], eng.dst[a:a + b]))
        ranks.append(eng.rank_events(a, b, candidates, exclude_seen=exclude_seen, exclude_self=exclude_self,
                                     cached=cached, exclude_history=exclude_history, history_since=history_since)[0])
    rank = torch.cat(ranks) if ranks else torch.zeros(0, dtype=torch.float64, device=eng.dev)
    stats = torch.stack([torch.nan_to_num(1.0 / rank, nan=0.0).sum()] + [(rank <= k).sum().double() for k in ks])
    stats = (stats / max(hi - lo, 1)).tolist()
    out = {"mrr": stats[0], "rank": rank}
    out.update({f"hits@{k}": v for k, v in zip(ks, stats[1:])})
    if split_history:                                        # (the parts' means are numpy's over the ranks read back)
        import numpy as np
        rep = torch.cat(reps) if reps else torch.zeros(0, dtype=torch.bool, device=eng.dev)
        out["repeat"] = rep
        r_host, m_host = rank.cpu().numpy(), rep.cpu().numpy()
        for name, m in (("repeat", m_host), ("novel", ~m_host)):
            part = r_host[m]
            n = int(part.size)
            out[f"n_{name}"] = n
            out[f"mrr_{name}"] = float(np.nan_to_num(1.0 / part, nan=0.0).mean()) if n else float("nan")
            out.update({f"hits@{k}_{name}": (float((part <= k).mean()) if n else float("nan")) for k in ks})
    return out


@torch.no_grad()
def embedding_table(model, neighbor_loader):
    """The [N, D] table of current eval-mode embeddings of the engine train() / test() attached to the model
    (TgnEngine.embedding_table; the table is enabled here if it is not, and only its stale rows are recomputed): the
    export for a downstream index.  A view that the next state change invalidates: clone() what must outlive it.
    Switches the memory to eval first as recommend() does."""
    eng = _bound_engine(model, neighbor_loader, "embedding_table")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    eng.enable_embedding_table()
    return eng.embedding_table()


@torch.no_grad()
def observe(model, neighbor_loader, src, dst, t, msg, batch=None):
    """Take new interactions into the stream state of the engine train() / test() attached to the model, without
    scoring them: the rows are appended to the resident event table, then memory, message stores and ring advance over
    them in batches of `batch` (default: the model's max_batch) exactly as test() batches would leave them
    (TgnEngine.observe_events; no negatives, no outputs).  Straight after train() the memory is switched to eval first,
    as test() and recommend() do.  Returns (start, n): the events are rows [start, start + n) of the table.  Rows that
    may name new nodes: observe_grow()."""
    return _observe(model, neighbor_loader, src, dst, t, msg, batch, False)


@torch.no_grad()
def observe_grow(model, neighbor_loader, src, dst, t, msg, batch=None):
    """observe() for interactions that may name nodes the model has not seen: node ids at or above its num_nodes are
    admitted — the node space grows to the largest id + 1 first (TgnEngine.grow_nodes; train() / test() capture their
    graphs again on their next call)."""
    return _observe(model, neighbor_loader, src, dst, t, msg, batch, True)


def _observe(model, neighbor_loader, src, dst, t, msg, batch, grow):
    eng = getattr(_owner(model), "_tgnx_engine", None)
    if eng is None or eng.loader is not neighbor_loader:
        raise RuntimeError("tgnx observe: no engine bound to this model / neighbor_loader yet (run train() or test() "
                           "first: they bind the event table)")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    start, n = eng.observe_events(src, dst, t, msg, batch=batch, grow=grow)
    neighbor_loader.cur_e_id = start + n
    return start, n


def _bound_engine(model, neighbor_loader, what):
    eng = getattr(_owner(model), "_tgnx_engine", None)
    if eng is None or eng.loader is not neighbor_loader:
        raise RuntimeError(f"tgnx {what}: no engine bound to this model / neighbor_loader yet (run train() or test() "
                           "first: they bind the event table)")
    return eng


@torch.no_grad()
def grow_nodes(model, neighbor_loader, n):
    """Extend the node space of the model, its neighbor_loader and the engine train() / test() attached to them to n
    nodes in place (TgnEngine.grow_nodes): old rows unchanged, new rows as reset_state leaves them, no parameter
    touched.  Before an engine exists the model and the loader are grown on their own.  Returns num_nodes afterwards.
    The engine's dst_nodes (the train negative pool) is not extended."""
    m = _owner(model)
    eng = getattr(m, "_tgnx_engine", None)
    if eng is not None and eng.loader is neighbor_loader:
        return eng.grow_nodes(n)
    if getattr(m, "_tgnx_grow", None) is not None and m._tgnx_grow() is not None:
        raise RuntimeError("tgnx grow_nodes: the model is bound to an engine over another neighbor_loader")
    neighbor_loader.grow(n)
    return m.grow_nodes(n)


@torch.no_grad()
def compact(model, neighbor_loader, upto=None, capacity=None):
    """Retire every row of the resident event table that neither the ring nor a message store references and renumber
    the survivors in order (TgnEngine.compact_events: rows >= upto are kept verbatim).  Returns kept, the surviving
    rows' old ids (kept[new] = old).  The stream state is unchanged, so nothing is flushed; the train / eval bindings
    and graphs of the loops above are dropped (their splits name rows that no longer exist): train() / test() over a
    loader of the new numbering bind again."""
    eng = _bound_engine(model, neighbor_loader, "compact")
    kept = eng.compact_events(upto=upto, capacity=capacity)
    neighbor_loader.cur_e_id = eng.num_events
    return kept


@torch.no_grad()
def forget(model, neighbor_loader, ids, compact=False, drop_candidates=False):
    """Erase the nodes `ids` from the stream state of the engine train() / test() attached to the model
    (TgnEngine.forget_nodes): their memory, stores and ring rows become a never-seen node's, every other node's ring
    slots and stored messages that name them are removed, and compact=True retires the event rows only they kept alive.
    What their past messages already did to their partners' memory stays.  Straight after train() the memory is
    switched to eval first, as observe() does (the flush folds the stored messages in; forgetting before it would only
    drop them).  drop_candidates=True also removes ids from the engine's dst_nodes.  Returns forget_nodes' counts.  The
    train / eval bindings and graphs of the loops above are dropped: train() / test() bind again."""
    eng = _bound_engine(model, neighbor_loader, "forget")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    out = eng.forget_nodes(ids, compact=compact, drop_candidates=drop_candidates)
    neighbor_loader.cur_e_id = eng.num_events
    return out


def _pair_history(data, device):
    """The PairHistory over a TemporalData's whole stream on `device`, built once and kept on the data object."""
    from .tgb_negs import PairHistory
    dev = torch.device(device)
    idx = getattr(data, "_tgnx_pair_hist", None)
    if idx is None or idx.num_rows != data.num_events or idx.device.type != dev.type:
        idx = PairHistory.build(data.src, data.dst, data.num_nodes, device=dev)
        data._tgnx_pair_hist = idx
    return idx


@torch.no_grad()
def tgb_negatives(loader, k, *, hist_ratio=0.5, hist_hi=None, pool=None, seed=0, device="cuda"):
    """TGB's hist_rnd evaluation negatives for a SplitLoader's split, generated on the device from the stream's float64
    timestamps (tgnx.tgb_negs.tgb_negatives: per event int(k * hist_ratio) destinations its source met before the split
    and is not meeting now, the rest random destinations that are neither) and installed as loader.negatives, so that
    test() takes the resident pass on them.  Returns the [hi - lo, k] table (on the device)."""
    from .tgb_negs import tgb_negatives as generate
    if not isinstance(loader, SplitLoader):
        raise TypeError("tgnx tgb_negatives needs a tgnx.data.SplitLoader")
    d = loader.data
    negs = generate(d.src, d.dst, d.t.double(), loader.lo, loader.hi, k, hist_ratio=hist_ratio, hist_hi=hist_hi,
                    pool=pool, seed=seed, index=_pair_history(d, device))
    loader.negatives = negs
    loader._dev = {}                                      # (resident() caches the negatives it moved)
    return negs


@torch.no_grad()
def edgebank(loader, batch=None, device="cuda"):
    """The MRR of EdgeBank-inf (TGB's memorisation baseline: a pair scores 1 if it occurred before the start row of its
    batch, else 0) over a SplitLoader's split under loader.negatives, in batches of `batch` (default: the loader's):
    the number to hold a model's test() MRR on the same negatives against.  Two PairHistory.contains calls plus
    torch (tgnx.tgb_negs.edgebank_mrr)."""
    from .tgb_negs import edgebank_mrr
    negs = loader.negatives
    if not (torch.is_tensor(negs) and negs.dim() == 2 and negs.shape[0] == loader.hi - loader.lo):
        raise ValueError("tgnx edgebank needs a rectangular negatives table on the loader ([hi - lo, K])")
    d = loader.data
    return edgebank_mrr(_pair_history(d, device), d.src, d.dst, negs, loader.lo, loader.hi,
                        loader.batch_size if batch is None else int(batch))


def edgebank_window(t_train, ratio=0.15) -> float:
    """The duration of EdgeBank-tw's window as TGB's default states it: `ratio` (0.15) of the span of the training
    timestamps."""
    t = torch.as_tensor(t_train).double()
    if t.numel() == 0 or not 0.0 < ratio <= 1.0:
        raise ValueError("edgebank_window: empty timestamps, or ratio outside (0, 1]")
    return float((t.max() - t.min()) * ratio)


@torch.no_grad()
def edgebank_stream(loader, lo, hi, batch, negs, window=None, device="cuda"):
    """Prequential EdgeBank over rows [lo, hi) of a stream from a live tgnx.pairset.PairSet: the bank is loaded with rows
    [0, lo), then every batch of `batch` events has its positives and its negatives (negs [hi - lo, K]) scored against
    the bank as it stood before the batch, and is inserted.  window=None is EdgeBank-inf (score 1 for a pair the bank
    holds); with a window (a duration, edgebank_window) a pair scores 1 iff t_last >= t_hi - window, t_hi the largest
    float32 stamp inserted so far, the difference taken in float32 (EdgeBank-tw; before anything is inserted nothing
    scores).  loader: a SplitLoader or anything with .src / .dst / .t (stamps are taken as float32, the event table's
    type).  Ranks are tie-averaged and the result is the mean over batches of the batch MRR, as
    tgnx.tgb_negs.edgebank_mrr reports it; window=None equals it exactly on the same negatives.  Host reads: the
    PairSet's growth schedule and one at the end."""
    import numpy as np

    from .pairset import PairSet, min_capacity
    d = getattr(loader, "data", loader)
    lo, hi, batch = int(lo), int(hi), int(batch)
    dev = torch.device(device)
    src, dst = torch.as_tensor(d.src).to(dev, torch.long), torch.as_tensor(d.dst).to(dev, torch.long)
    t_host = torch.as_tensor(d.t).to(torch.float32).cpu()
    t = t_host.to(dev)
    E = int(src.numel())
    negs = torch.as_tensor(negs).to(dev, torch.long)
    if not (0 <= lo <= hi <= E) or batch <= 0 or negs.dim() != 2 or negs.shape[0] != hi - lo:
        raise ValueError(f"edgebank_stream: rows [{lo}, {hi}) batch {batch} outside the {E}-event stream, or negs is "
                         f"not [hi - lo, K]")
    if window is not None and not float(window) >= 0.0:
        raise ValueError("edgebank_stream: window must be a duration >= 0")
    n, K = hi - lo, int(negs.shape[1])
    if n == 0:
        return float("nan")
    num_nodes = int(max(int(src.max()), int(dst.max()), int(negs.max()) if negs.numel() else 0)) + 1
    bank = PairSet(num_nodes, min_capacity(batch), device=dev)
    bank.insert(src[:lo], dst[:lo], t[:lo])
    t_np = t_host.numpy()
    t_hi = np.float32(t_np[:lo].max()) if lo else None
    rrs = []
    for a in range(lo, hi, batch):
        b = min(batch, hi - a)
        s, p, ng = src[a:a + b], dst[a:a + b], negs[a - lo:a - lo + b]
        if window is None:
            since = None
        elif t_hi is None:
            since = float("inf")
        else:
            since = float(np.float32(t_hi - np.float32(window)))
        pos = bank.contains(s, p, since).double()
        neg = bank.contains(s.repeat_interleave(K), ng.reshape(-1), since).view(b, K).double()
        rank = 0.5 * ((neg > pos[:, None]).sum(1) + (neg >= pos[:, None]).sum(1)).double() + 1.0
        rrs.append(1.0 / rank)
        bank.insert(s, p, t[a:a + b])
        m = np.float32(t_np[a:a + b].max())
        t_hi = m if t_hi is None else max(t_hi, m)
    rr = torch.cat(rrs).cpu().numpy()
    return float(np.mean([rr[a:a + batch].mean() for a in range(0, n, batch)]))


@torch.no_grad()
def enable_pair_history(model, neighbor_loader, capacity=None):
    """Turn on the live pair history of the engine train() / test() attached to the model
    (TgnEngine.enable_pair_history): observe() and the per-batch test path record their batches from here on; rows
    trained or validated by the resident passes are recorded with the engine's record_pairs(lo, hi)."""
    _bound_engine(model, neighbor_loader, "enable_pair_history").enable_pair_history(capacity)


@torch.no_grad()
def seen(model, neighbor_loader, src, dst, since=None):
    """bool[n] on the device: has src[i] ever interacted with dst[i] in the recorded stream (TgnEngine.seen)."""
    return _bound_engine(model, neighbor_loader, "seen").seen(src, dst, since)


@torch.no_grad()
def save_stream(model, neighbor_loader, f):
    """torch.save the engine's stream state (TgnEngine.stream_state; no parameters: the model's state_dict() has them)
    to the path or file object f.  Straight after train() the memory is switched to eval first, as test(), recommend()
    and observe() do, so the file holds a serving state.  Small when taken after compact().  With the pair history
    enabled the file also carries it under "pair_history" (TgnEngine.pair_history_state, moved to the host);
    stream_state()'s own keys and format are unchanged, and TgnEngine.load_stream_state reads its own keys only, so it
    takes such a file as it is (ignoring the history: load_stream carries it)."""
    eng = _bound_engine(model, neighbor_loader, "save_stream")
    if eng._mode_train:
        eng.flush()
        eng._mode_train = False
    state = eng.stream_state()
    if eng._pairs is not None:
        ph = eng.pair_history_state()
        state["pair_history"] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ph.items()}
    torch.save(state, f)


@torch.no_grad()
def load_stream(model, neighbor_loader, f, optimizer=None, dst_nodes=None):
    """Load a save_stream file into the engine attached to the model — or, in a fresh process where none is, into a
    new engine over a one-row table (optimizer and dst_nodes as train() would have given it) — and leave it in eval
    mode: observe(), recommend() and test() go on from the saved state (TgnEngine.load_stream_state).  A file that
    carries a pair history enables it and loads it; a file without one leaves an enabled history empty."""
    m = _owner(model)
    eng = getattr(m, "_tgnx_engine", None)
    state = torch.load(f, map_location="cpu")
    if eng is None or eng.loader is not neighbor_loader:
        d = m.cfg.msg_dim
        eng = TgnEngine(m, neighbor_loader, dict(src=torch.zeros(1, dtype=torch.long), dst=torch.zeros(1, dtype=torch.long),
                                                 t=torch.zeros(1), msg=torch.zeros(1, d)), optimizer,
                        dst_nodes=None if dst_nodes is None else torch.as_tensor(dst_nodes))
        eng.out_ev = torch.zeros(eng.cfg.num_events, 2, dtype=torch.float32, device=eng.dev)
        eng.keep_grads = False
        eng._bound = None
        m._tgnx_engine = eng
    ph = state.pop("pair_history", None)
    eng.load_stream_state(state)
    if ph is not None:
        eng.load_pair_history_state(ph)
    elif eng._pairs is not None:
        eng.clear_pair_history()
    eng._mode_train = False
    neighbor_loader.cur_e_id = eng.num_events
    return eng.num_events
