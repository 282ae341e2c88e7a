"""GPU tests of read-only TGN inference: TgnEngine.embed / recommend over tgnx_tgn_embed and the fused top-k
operator, and the drop-in tgn_epoch.recommend.

Setup: a 600-event wiki-shaped stream over 300 nodes (msg_dim 16, D = 32, ring 10), parameters from a RefTGN state
dict, dropout 0.  The state is built with EVAL batches only — 6 x eval_batch on the engine and
oracle.tgn_ref.eval_step on the oracle with the same negatives — so the parameters never move and both sides stay
deterministic (the engine is flushed once from the reset state first, as the oracle's first eval() flushes its
empty stores: memory_module.py:209-215 sends every node's row through the updater).  layers in {1, 2} x aggr in
{last, mean}.

  parity     embed(120 nodes: duplicates, a node with an empty ring row, the hub) against the oracle's eval forward
             for the same set (oracle/tgn_ref.py eval_step: sample_hops -> memory(n_id) in eval mode -> gnn), 2e-5 in
             the `_close` metric (max |a - b| over max(|b|, 1)): the bound test_gpu_nn_modules.py holds the same
             quantity to;
  chunking   an engine of capacity 24 roots (max_batch 8, max_neg 1) embeds the 120 nodes in 5 chunks within the same
             bound (no bit-equality between chunkings: GEMM split choices depend on the row count); capacity + 1
             nodes in one C call is TGNX_EINVAL;
  invalid    embed([-1, N]) raises; the C call counts them, zero-fills their rows, leaves the valid rows correct;
  read-only  memory, last_update, stores, ring, parameters, Adam moments and every ctl word but GEN bit-identical
             after embed + recommend; GEN grew by the number of C calls; ERR is 0;
  eval goes on unchanged     twin engines, one with embed / recommend between two further eval batches: outputs and
             reciprocal ranks torch.equal;
  train goes on unchanged    twin resident engines (gather-ahead and parity sets on), 4 steps, one with a recommend
             after step 2: ring, stores, last_update exact; memory within 1e-4 and parameters within 2e-5, the
             run-to-run bounds test_gpu_tgn_rccl.py documents for the step's float atomics; the batch counter equal;
  recommend  logits against the oracle's all-pairs logits at 2e-5; node ids = candidates[stable top-k of the returned
             logits] exactly; the default candidate set; padding;
  drop-in    tgn_epoch.recommend after tgn_epoch.train flushes once and equals engine.recommend on a twin flushed by
             hand."""
import ctypes

import numpy as np
import pytest
import torch

from tgn_oracle_steps import oracle_embed as _oracle_embed  # (the oracle's eval forward for a node set)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, d, D, B, KN, NEV = 300, 16, 32, 50, 5, 600
TOL = 2e-5
FORMS = [(1, "last"), (1, "mean"), (2, "last"), (2, "mean")]


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _stream():
    from tgnx.synth import make_stream
    return make_stream("tgbl-wiki", seed=5, num_events=NEV, num_nodes=N, msg_dim=d)


def _engine(s, sd, layers, aggr, max_batch=B, max_neg=KN, dst_nodes=True):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    model = TGNModel(N, s.num_events, d, D, DEV, ring=10, max_batch=max_batch, max_neg=max_neg, aggr=aggr, dropout=0.0,
                     layers=layers)
    model.load_reference_state(sd)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=DEV),
                    dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), TgnAdam(model, 1e-3),
                    dst_nodes=s.dst_nodes if dst_nodes else None, seed=7)
    eng.reset_state()
    return eng


def _ref(layers, aggr):
    from oracle.tgn_ref import RefTGN
    torch.manual_seed(0)
    return RefTGN(N, d, hidden=D, aggr=aggr, dropout=0.0, layers=layers)


def _negs(s, batch, kn):
    return torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(8 * batch, kn)))


def _eval_batches(eng, s, negs, batch, first, count):
    out = []
    for st in range(first, first + count):
        p, n, r = eng.eval_batch(st * batch, batch, negs[st * batch:(st + 1) * batch])
        out.append((p.clone(), n.clone(), r.clone()))
    torch.cuda.synchronize()
    eng.check()
    return out


def _oracle_state(ref, s, negs, batch, count):
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import eval_step
    lref = RefLastNeighborLoader(N, 10)
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    src, dst = torch.from_numpy(s.src), torch.from_numpy(s.dst)
    for st in range(count):
        sl = slice(st * batch, (st + 1) * batch)
        eval_step(ref, lref, ev_t, ev_msg, src[sl], dst[sl], negs[sl], ev_t[sl], ev_msg[sl])
    return lref, ev_t, ev_msg


def _query_nodes(s, events):
    """120 nodes: the hub, a node without history (an empty ring row), duplicates of both and of random ones."""
    seen = np.concatenate([s.src[:events], s.dst[:events]])
    hub = int(np.bincount(seen, minlength=N).argmax())
    empty = int(np.setdiff1d(np.arange(N), seen)[0])
    rnd = np.random.default_rng(3).integers(0, N, 114)
    return np.concatenate([[hub, empty, hub], rnd, [empty, int(rnd[0]), int(rnd[1])]]).astype(np.int64), hub, empty


_BUILT = {}


def _built(layers, aggr, batch=B, kn=KN):
    """(stream, engine, oracle model, oracle loader, ev_t, ev_msg, negatives) after 6 eval batches on both sides;
    built once per configuration.  Tests that move the engine's state build their own."""
    key = (layers, aggr, batch, kn)
    if key not in _BUILT:
        s = _stream()
        ref = _ref(layers, aggr)
        eng = _engine(s, ref.state_dict(), layers, aggr, max_batch=batch, max_neg=kn)
        eng.flush()     # the oracle's first eval() is TGNMemory.train(False): every node's row through the updater once
        negs = _negs(s, batch, kn)
        _eval_batches(eng, s, negs, batch, 0, 6)
        lref, ev_t, ev_msg = _oracle_state(ref, s, negs, batch, 6)
        _BUILT[key] = (s, eng, ref, lref, ev_t, ev_msg, negs)
    return _BUILT[key]


def _embed_c(eng, nodes, n=None):
    """tgnx_tgn_embed called directly: (rc, out [n, D] pre-filled with NaN, n_invalid)."""
    from tgnx import _lib
    nodes = torch.as_tensor(nodes, dtype=torch.long).to(DEV).contiguous()
    n = nodes.numel() if n is None else n
    out = torch.full((n, D), float("nan"), device=DEV)
    cnt = torch.zeros(1, dtype=torch.long, device=DEV)
    b = eng._buffers(0)
    rc = _lib.lib().tgnx_tgn_embed(ctypes.byref(eng.cfg), ctypes.byref(b), ctypes.c_void_p(nodes.data_ptr()), n,
                                   ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(cnt.data_ptr()), eng._stream())
    torch.cuda.synchronize()
    return rc, out, int(cnt)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_embed_matches_the_oracle_eval_forward(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    nodes, hub, empty = _query_nodes(s, 6 * B)
    assert int((eng.loader.e_id[empty] >= 0).sum()) == 0 and int((eng.loader.e_id[hub] >= 0).sum()) == 10
    z = eng.embed(nodes)
    assert z.shape == (120, D) and z.dtype == torch.float32
    _close(z, _oracle_embed(ref, lref, ev_t, ev_msg, nodes), TOL)
    assert torch.equal(z[0], z[2]) and torch.equal(z[1], z[117])          # duplicates: the same row
    assert torch.equal(eng.embed(torch.from_numpy(nodes)), z)            # and the same again
    assert eng.embed([]).shape == (0, D)


@pytest.mark.parametrize("layers,aggr", FORMS)
def test_embed_in_chunks(layers, aggr):
    from tgnx import _lib
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr, batch=8, kn=1)
    assert eng.embed_capacity() == 24
    nodes, _, _ = _query_nodes(s, 6 * 8)
    gen0 = int(eng.ctl[3])
    z = eng.embed(nodes)
    assert int(eng.ctl[3]) - gen0 == 5                                     # 120 nodes, 24 per call
    _close(z, _oracle_embed(ref, lref, ev_t, ev_msg, nodes), TOL)
    rc, _, _ = _embed_c(eng, nodes[:25])
    assert rc == -1 and b"tgnx_tgn_embed" in _lib.lib().tgnx_last_error()  # TGNX_EINVAL
    assert int(eng.ctl[3]) - gen0 == 5                                     # refused before any launch


def test_invalid_ids():
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(1, "last")
    with pytest.raises(ValueError):
        eng.embed([3, -1, 7])
    with pytest.raises(ValueError):
        eng.embed([N])
    rc, out, bad = _embed_c(eng, [3, -1, 7, N, 3])
    assert rc == 0 and bad == 2
    assert bool((out[1] == 0).all()) and bool((out[3] == 0).all())
    _close(out[[0, 2, 4]], _oracle_embed(ref, lref, ev_t, ev_msg, [3, 7, 3]), TOL)
    z = eng.embed([3, -1, 7], validate=False)                              # unvalidated: a zero row, no error flag
    assert bool((z[1] == 0).all()) and torch.equal(z[[0, 2]], out[[0, 2]])
    eng.check()


def _state(eng):
    m, ld = eng.model, eng.loader
    return dict(memory=m.memory.memory, last_update=m.memory.last_update, store=m.store, node_gen=m.node_gen,
                neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t, flat=m.flat, grad=m.grad_flat, adam_m=eng.adam_m,
                adam_v=eng.adam_v, ctl=eng.ctl)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_embed_and_recommend_change_nothing(layers, aggr):
    s, eng, *_ = _built(layers, aggr)
    nodes, _, _ = _query_nodes(s, 6 * B)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(eng).items()}
    cap = eng.embed_capacity()
    assert cap == min(N, B * (2 + KN))
    eng.embed(nodes)
    src = torch.from_numpy(s.src[:7].copy())
    eng.recommend(src, 5)
    eng.recommend(src, 5, candidates=np.arange(40))
    torch.cuda.synchronize()
    calls = -(-120 // cap) + -(-(7 + len(s.dst_nodes)) // cap) + -(-47 // cap)
    after = _state(eng)
    for k, v in before.items():
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]
            assert torch.equal(after[k][keep], v[keep]), (k, after[k].tolist(), v.tolist())
            assert int(after[k][3]) - int(v[3]) == calls
            assert int(after[k][11]) == 0
        else:
            assert torch.equal(_bits(after[k]), _bits(v)), k


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "last")])
def test_eval_goes_on_unchanged(layers, aggr):
    s = _stream()
    sd = _ref(layers, aggr).state_dict()
    negs = _negs(s, B, KN)
    a, b = (_engine(s, sd, layers, aggr) for _ in range(2))
    for e in (a, b):
        _eval_batches(e, s, negs, B, 0, 6)
    nodes, _, _ = _query_nodes(s, 6 * B)
    ra = _eval_batches(a, s, negs, B, 6, 1)
    a.embed(nodes)
    a.recommend(nodes[:9], 10)
    ra += _eval_batches(a, s, negs, B, 7, 1)
    a.embed(nodes[:5])
    rb = _eval_batches(b, s, negs, B, 6, 2)
    for (pa, na, qa), (pb, nb, qb) in zip(ra, rb):
        assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(qa, qb)
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert torch.equal(_bits(_state(a)[k]), _bits(_state(b)[k])), k


def test_train_goes_on_unchanged_after_a_query_between_prefetched_steps():
    """The prefetch trap: a pipelined / parity-set / gather-ahead step has already prepared the NEXT batch in the
    workspace the query reuses; recommend() must make the next step prepare it again."""
    s = _stream()
    sd = _ref(1, "last").state_dict()
    a, b = (_engine(s, sd, 1, "last") for _ in range(2))
    for e in (a, b):
        assert e.gather_ahead and e.parity_sets
        e.bind_resident(0, NEV, B, dropout=False)
        e.begin_epoch()
    for step in range(4):
        a.resident_train_step()
        b.resident_train_step()
        if step == 1:
            assert a._prefetched
            a.recommend(torch.from_numpy(s.src[:7].copy()), 5)
            assert not a._prefetched
    torch.cuda.synchronize()
    a.check()
    b.check()
    sa, sb = _state(a), _state(b)
    for k in ("neighbors", "e_id", "t", "store", "last_update"):
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), k
    _close(sa["memory"], sb["memory"], 1e-4)
    _close(sa["flat"], sb["flat"], 2e-5)
    assert int(a.ctl[10]) == int(b.ctl[10]) == 4                           # TGNX_CTL_NB
    assert int(a.ctl[4]) == int(b.ctl[4])                                  # the optimizer step count
    assert abs(a.loss_sum() - b.loss_sum()) <= 1e-4 * abs(b.loss_sum())


def _stable_topk_ids(logits, cand, k):
    ids = np.full((logits.shape[0], k), -1, dtype=np.int64)
    for q in range(logits.shape[0]):
        order = np.lexsort((np.arange(logits.shape[1]), -logits[q]))[:k]
        ids[q, :order.size] = cand[order]
    return ids


@pytest.mark.parametrize("layers,aggr", [(1, "last"), (2, "mean")])
def test_recommend(layers, aggr):
    s, eng, ref, lref, ev_t, ev_msg, _ = _built(layers, aggr)
    rng = np.random.default_rng(4)
    src = rng.integers(0, N, 7)
    cand = rng.permutation(N)[:90]
    cand[50] = cand[10]                                                    # a duplicate candidate
    val, ids, logits = eng.recommend(src, 5, candidates=cand, return_scores=True)
    assert val.shape == ids.shape == (7, 5) and logits.shape == (7, 90)
    z = _oracle_embed(ref, lref, ev_t, ev_msg, np.concatenate([src, cand]))
    lp = ref.link_pred
    with torch.no_grad():
        want = lp.lin_final((lp.lin_src(z[:7])[:, None] + lp.lin_dst(z[7:])[None]).relu()).squeeze(-1)
    _close(logits, want, TOL)
    lg = logits.cpu().numpy()
    assert np.array_equal(ids.cpu().numpy(), _stable_topk_ids(lg, cand, 5))
    assert np.array_equal(lg[:, 50], lg[:, 10])                           # the duplicate scores the same ...
    top = np.sort(lg, axis=1)[:, ::-1][:, :5]
    assert float((val.cpu() - torch.sigmoid(torch.from_numpy(top.copy()))).abs().max()) <= 1e-6
    # the default candidate set: the engine's destination nodes, else every node
    v1, i1 = eng.recommend(src, 5)
    v2, i2 = eng.recommend(src, 5, candidates=eng.dst_nodes)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    assert bool(torch.isin(i1, eng.dst_nodes).all())
    saved = eng.dst_nodes
    try:
        eng.dst_nodes = None
        v3, i3 = eng.recommend(src, 5)
    finally:
        eng.dst_nodes = saved
    v4, i4 = eng.recommend(src, 5, candidates=torch.arange(N))
    assert torch.equal(i3, i4) and torch.equal(v3, v4)
    # more slots than candidates: node id -1, value 0
    v5, i5 = eng.recommend(src, 8, candidates=cand[:5])
    assert bool((i5[:, 5:] == -1).all()) and bool((v5[:, 5:] == 0).all())
    assert np.array_equal(np.sort(i5[:, :5].cpu().numpy(), axis=1), np.tile(np.sort(cand[:5]), (7, 1)))
    with pytest.raises(ValueError):
        eng.recommend([N], 3)
    eng.check()


def test_dropin_recommend_flushes_once_and_equals_a_hand_flushed_twin():
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
    model = TGNModel(N, NEV, d, D, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(sd)
    nl = LastNeighborLoader(N, 10, device=DEV)
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.recommend(model, nl, [1, 2], 3)
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train
    stores = lambda m: int(m.store[:4 * N].view(N, 4)[:, [1, 3]].sum())  # noqa: E731
    assert stores(model) > 0
    # the twin: an engine of its own in the same post-train state, flushed by hand
    twin = _engine(s, sd, 1, "last")
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(twin).items():
            if k not in ("grad", "adam_m", "adam_v"):
                v.copy_(_state(eng)[k])
    twin.flush()
    src = torch.from_numpy(s.src[200:212].copy())
    want = twin.recommend(src, 6)
    got = pyg_epoch_utils.recommend(model, nl, src, 6)
    assert not eng._mode_train and stores(model) == 0                      # switched to eval: flushed
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    mem = model.memory.memory.clone()
    again = tgn_epoch.recommend(model, nl, src, 6, candidates=twin.dst_nodes)
    assert torch.equal(model.memory.memory, mem)                           # no second flush, nothing written
    assert torch.equal(again[1], want[1]) and torch.equal(again[0], want[0])
