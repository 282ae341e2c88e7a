"""GPU tests of the hist_rnd evaluation negatives' surfaces: TgnEngine.pair_history / eval_negatives, the drop-in's
pyg_epoch_utils.tgb_negatives (the table installed on a SplitLoader, test() taking the resident pass on it) and
pyg_epoch_utils.edgebank (EdgeBank-inf under the loader's negatives) against a numpy EdgeBank."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, d, D, B = 600, 16, 32, 50
E, LO, HI = 1200, 800, 1130


def _engine(s):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = TGNModel(N, s.num_events, d, D, dev, ring=10, max_batch=B, max_neg=20)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=dev), dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32),
                    msg=s.msg), TgnAdam(model, 1e-3), dst_nodes=s.dst_nodes, seed=7)
    eng.reset_state()
    return eng


def test_engine_eval_negatives_equal_tgb_negatives():
    """eval_negatives on the resident table == tgb_negatives on the same arrays (float32 t, the engine's dst_nodes as
    the pool); the index is kept while num_events stands, rebuilt after append_events, dropped by compact_events."""
    from tgnx.synth import make_stream
    from tgnx.tgb_negs import tgb_negatives
    s = make_stream("tgbl-wiki", seed=5, num_events=E, num_nodes=N, msg_dim=d)
    eng = _engine(s)
    got = eng.eval_negatives(LO, HI, 20, seed=3)
    want, kh, st = tgb_negatives(s.src, s.dst, s.t.astype(np.float32), LO, HI, 20, pool=np.unique(s.dst_nodes), seed=3,
                                 return_info=True)
    assert got.is_cuda and tuple(got.shape) == (HI - LO, 20) and torch.equal(got, want)
    assert int(kh.max()) > 0 and st[0] == -1                 # the stream repeats pairs: historical picks exist
    idx = eng.pair_history()
    assert eng.pair_history() is idx and idx.num_rows == E
    seen = idx.contains(s.src[:LO], s.dst[:LO], before=LO)
    assert bool(seen.all())
    eng.append_events(s.src[:5], s.dst[:5], s.t[-1] + 1 + np.arange(5, dtype=np.float32), s.msg[:5])
    idx2 = eng.pair_history()
    assert idx2 is not idx and idx2.num_rows == E + 5
    eng.observe_range(0, E + 5, B)
    eng.compact_events()
    assert "_pair_hist" not in eng.__dict__ and 0 < eng.num_events < E + 5
    assert eng.pair_history().num_rows == eng.num_events
    eng.check()


def _np_edgebank(src, dst, negs, lo, hi, batch):
    perf = []
    for a in range(lo, hi, batch):
        b = min(hi, a + batch)
        bank = set(zip(src[:a].tolist(), dst[:a].tolist()))
        pos = np.array([(int(s), int(x)) in bank for s, x in zip(src[a:b], dst[a:b])], np.float64)
        neg = np.array([[(int(s), int(x)) in bank for x in row] for s, row in zip(src[a:b], negs[a - lo:b - lo])], np.float64)
        rank = 0.5 * ((neg > pos[:, None]).sum(1) + (neg >= pos[:, None]).sum(1)) + 1.0
        perf.append((1.0 / rank).mean())
    return float(np.mean(perf))


def test_dropin_negatives_resident_pass_and_edgebank(monkeypatch):
    """pyg_epoch_utils.tgb_negatives(val_loader, 20) installs a [n, 20] table (== tgb_negatives on the loader's float64
    stream), test() runs the resident pass on it and returns the mean of eval_batch's reciprocal ranks over the same
    table on a twin engine in the same state (the same float, as tests/test_gpu_tgn_eval_resident.py compares them);
    edgebank(loader) == a numpy EdgeBank over the same negatives exactly."""
    monkeypatch.setenv("TGNX_SYNTH_EVENTS", "3000")
    monkeypatch.setenv("TGNX_EVAL_NEGS", "30")
    import pyg_epoch_utils as pe
    import pyg_model_utils as pm
    from tgnx.data import getDataWithDependecyBlock
    from tgnx.neg import NegLinkSamplerDest
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgb_negs import tgb_negatives
    from tgnx.tgn import TgnEngine
    data, tr, va, te, ns, ev, metric = getDataWithDependecyBlock("tgbl-wiki", {"batch_size": 200})
    assert tuple(va.negatives.shape) == (va.hi - va.lo, 30)          # (the uniform default is untouched)
    negs = pe.tgb_negatives(va, 20, seed=4)
    assert va.negatives is negs and negs.is_cuda and tuple(negs.shape) == (va.hi - va.lo, 20)
    want_negs, kh, st = tgb_negatives(data.src, data.dst, data.t.double(), va.lo, va.hi, 20, seed=4, return_info=True)
    assert torch.equal(negs, want_negs) and int(kh.max()) > 0
    src, dst = data.src.numpy(), data.dst.numpy()
    nn = negs.cpu().numpy()
    assert not (nn == dst[va.lo:va.hi, None]).any()                   # never the positive
    # EdgeBank under these negatives, and under other batch sizes (the partial last batch included)
    for batch in (None, 64, va.hi - va.lo):
        got = pe.edgebank(va, batch=batch)
        assert got == _np_edgebank(src, dst, nn, va.lo, va.hi, batch or 200), batch
    assert 0.0 < pe.edgebank(va) <= 1.0
    # a trained model's test() on the installed table: the resident pass, equal to the per-batch loop on a twin
    dm, Dh, Nn = data.msg.shape[1], 100, data.num_nodes
    torch.manual_seed(0)
    model = pm.getModel(dm, Dh, Nn, "cuda", ring=10, max_batch=200, dropout=0.1)
    opt = pm.getOptimizer(model, 1e-4)
    nl = LastNeighborLoader(Nn, 10, device="cuda")
    nds = NegLinkSamplerDest(torch.unique(data.dst), device="cuda")
    crit = torch.nn.BCEWithLogitsLoss()
    pe.train(model, data.msg, tr, nl, nds, None, "cuda", opt, crit)
    eng = model["model"]._tgnx_engine
    m2 = pm.getModel(dm, Dh, Nn, "cuda", ring=10, max_batch=200, dropout=0.1)
    e2 = TgnEngine(m2["model"], LastNeighborLoader(Nn, 10, device="cuda"),
                   dict(src=data.src, dst=data.dst, t=data.t.float(), msg=data.msg.float()), pm.getOptimizer(m2, 1e-4),
                   dst_nodes=torch.unique(data.dst))
    e2.reset_state()
    eng.finish()
    torch.cuda.synchronize()
    pairs = lambda e: dict(flat=e.model.flat, memory=e.model.memory.memory, last_update=e.model.memory.last_update,  # noqa: E731
                           store=e.model.store, node_gen=e.model.node_gen, neighbors=e.loader.neighbors,
                           e_id=e.loader.e_id, t=e.loader.t, assoc=e.loader._assoc, ctl=e.ctl)
    with torch.no_grad():
        for key, v in pairs(e2).items():
            v.copy_(pairs(eng)[key])
    e2.loader.cur_e_id = eng.loader.cur_e_id
    e2.invalidate_prefetch()
    e2.flush()
    perf = []
    for a in range(va.lo, va.hi, 200):
        b = min(va.hi, a + 200)
        perf.append(e2.eval_batch(a, b - a, negs[a - va.lo:b - va.lo])[2].clone().mean())
    want = float(torch.stack(perf).mean())
    calls = []
    bind = eng.bind_eval_resident
    monkeypatch.setattr(eng, "bind_eval_resident", lambda *a, **k: (calls.append(a[3]), bind(*a, **k))[1])
    got = pe.test(model, data.msg, va, nl, ns, None, "cuda", opt, crit, ev, metric, "val")
    assert got == want, (got, want)
    assert len(calls) == 1 and calls[0] is negs and eng._ev[3] == 20
    assert 0.0 < got <= 1.0


def test_neg_strategy_env_generates_hist_rnd_tables(monkeypatch):
    """TGNX_EVAL_NEG_STRATEGY=hist_rnd: the loaders of a stream without tables carry tgb_negatives' rows (history =
    everything before each split; seeds 1 / 2 as the uniform tables use); unset, the uniform tables are unchanged."""
    from tgnx.data import getDataWithDependecyBlock
    from tgnx.tgb_negs import tgb_negatives
    monkeypatch.setenv("TGNX_SYNTH_EVENTS", "3000")
    monkeypatch.setenv("TGNX_EVAL_NEGS", "20")
    monkeypatch.delenv("TGNX_EVAL_NEG_STRATEGY", raising=False)
    uni = getDataWithDependecyBlock("tgbl-wiki", {"batch_size": 200})[2].negatives
    monkeypatch.setenv("TGNX_EVAL_NEG_STRATEGY", "hist_rnd")
    data, tr, va, te, ns, ev, metric = getDataWithDependecyBlock("tgbl-wiki", {"batch_size": 200})
    for ld, seed in ((va, 1), (te, 2)):
        want = tgb_negatives(data.src, data.dst, data.t, ld.lo, ld.hi, 20, seed=seed)
        assert tuple(ld.negatives.shape) == (ld.hi - ld.lo, 20) and torch.equal(ld.negatives, want.cpu())
    assert not torch.equal(va.negatives, uni)
    monkeypatch.delenv("TGNX_EVAL_NEG_STRATEGY")
    assert torch.equal(getDataWithDependecyBlock("tgbl-wiki", {"batch_size": 200})[2].negatives, uni)
