"""GPU tests of the explanation of a link score: TgnEngine.attention / explain over tgnx_tgn_explain and the
leave-one-out logit operator, and the drop-in explain / explain_recommendations.

Setup (explain_ref.py): tgn_oracle_steps.Rig with N = 300, B = 50, d = 16, stream seed 3, aggr "last"; the engine is
flushed once, then 8 eval batches with 5 negatives run on both sides (test_gpu_tgn_query._built's recipe); the 50 pairs
of batch 8 are explained.  (D, ring) in {(32, 10), (100, 10), (32, 3)}.  The reference is the STRUCTURAL one: the
oracle's eval forward on a copy of its loader with the removed slots' e_id set to -1, and RefLinkPredictor's layers
before the sigmoid.  Slots are aligned by event id, not by position.

Tolerances are the project's: z, loo_z, alpha 2e-5 (TOL of test_gpu_tgn_query.py), logit 2e-5 (OUT_TOL), effects 4e-5
(two logits).  As a condition on the input, not on the code, the oracle's own source-side slot effects must have a
median above 1e-3."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import explain_ref as xr
from tgn_oracle_steps import OUT_TOL, Rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL, EFF_TOL = 2e-5, 4e-5
CASES = [(32, 10), (100, 10), (32, 3)]
EXTREMES = [(128, 32), (2, 1)]           # the widest and the narrowest memory and ring the engine accepts
_BUILT, _WANT = {}, {}


def _rig(D, ring, layers=1):
    rig = Rig(aggr="last", N=xr.N, B=xr.B, d=xr.MSG, D=D, nb=xr.NB, seed=xr.SEED, ring=ring, layers=layers,
              max_neg=xr.KN)
    negs = xr.negatives(rig.s)
    rig.eng.flush()        # the oracle's first eval() is TGNMemory.train(False)
    for st in range(xr.BATCHES):
        rig.eng.eval_batch(st * xr.B, xr.B, negs[st * xr.B:(st + 1) * xr.B])
    torch.cuda.synchronize()
    rig.eng.check()
    xr.advance(rig.ref, rig.lref, rig.s, negs)
    assert np.array_equal(rig.eng.loader.e_id.cpu().numpy(), rig.lref.e_id)
    rig.negs = negs
    return rig


def _built(D, ring, layers=1):
    """The rig after the 8 eval batches, built once per configuration; tests that move its state build their own."""
    if (D, ring, layers) not in _BUILT:
        _BUILT[(D, ring, layers)] = _rig(D, ring, layers)
    return _BUILT[(D, ring, layers)]


def _want(D, ring, by):
    """The structural reference of the 50 pairs, computed once and left unchanged."""
    if (D, ring, by) not in _WANT:
        rig = _built(D, ring)
        src, dst = xr.pairs(rig.s)
        _WANT[(D, ring, by)] = xr.structural_explain(rig.ref, rig.lref, rig.ev_t, rig.ev_msg, src, dst, by)
    return _WANT[(D, ring, by)]


def _nodes(rig):
    src, dst = xr.pairs(rig.s)
    return np.unique(np.concatenate([src, dst]))


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _check_rows(rig, nodes, o):
    """count / neighbour / event / t of attention() or explain() rows against the oracle loader's rows, exactly."""
    lref, K = rig.lref, rig.ring
    valid = lref.e_id[nodes] >= 0
    cnt = valid.sum(1)
    assert np.array_equal(o["count"].cpu().numpy(), cnt)
    for name, tab, fill in (("neighbour", lref.neighbors, -1), ("event", lref.e_id, -1), ("t", lref.t, 0)):
        want = np.full((len(nodes), K), fill, dtype=tab.dtype)
        for r, v in enumerate(nodes):
            want[r, :cnt[r]] = tab[v][valid[r]]
        assert np.array_equal(o[name].cpu().numpy(), want), name
    return cnt


@pytest.mark.parametrize("D,ring,layers", [(D, r, 1) for D, r in CASES] + [(32, 10, 2)])
def test_attention_matches_the_oracle(D, ring, layers):
    rig = _built(D, ring, layers)
    eng = rig.eng
    nodes = np.concatenate([_nodes(rig), _nodes(rig)[:3]])                 # duplicates allowed
    o = eng.attention(nodes)
    torch.cuda.synchronize()
    assert o["alpha"].shape == (len(nodes), ring, 2) and o["z"].shape == (len(nodes), D)
    cnt = _check_rows(rig, nodes, o)
    assert torch.equal(_bits(o["z"]), _bits(eng.embed(nodes)))
    want = xr.oracle_attention(rig.ref, rig.lref, rig.ev_t, rig.ev_msg, nodes)
    alpha, ev = o["alpha"].double().cpu().numpy(), o["event"].cpu().numpy()
    worst = 0.0
    for r, v in enumerate(nodes):
        assert not alpha[r, cnt[r]:].any()
        if cnt[r]:
            ref = np.stack([want[int(v)][int(e)] for e in ev[r, :cnt[r]]])
            worst = max(worst, float(np.abs(alpha[r, :cnt[r]] - ref).max()))
            assert np.abs(alpha[r].sum(0) - 1).max() <= 1e-5
    print(f"D={D} ring={ring} layers={layers}: alpha max err {worst:.3e}")
    assert worst <= TOL
    assert int(o["n_invalid"]) == 0


@pytest.mark.parametrize("by", ["slot", "neighbour"])
@pytest.mark.parametrize("D,ring", CASES + EXTREMES)
def test_explain_matches_the_structural_reference(D, ring, by):
    rig = _built(D, ring)
    want = _want(D, ring, by)
    oracle_eff = np.abs(np.array([e for row in _want(D, ring, "slot")["src"] for e in row.values()]))
    print(f"oracle: {oracle_eff.size} source-side slot effects, median {np.median(oracle_eff):.3e} max {oracle_eff.max():.3e}")
    if (D, ring) in CASES:
        assert np.median(oracle_eff) > 1e-3                                 # a condition on the input
    src, dst = xr.pairs(rig.s)
    o = rig.eng.explain(src, dst, by=by)
    torch.cuda.synchronize()
    P = len(src)
    assert o["logit"].shape == (P,) and o["src_effect"].shape == o["dst_effect"].shape == (P, ring)
    err = float(np.abs(o["logit"].double().cpu().numpy() - want["logit"]).max())
    print(f"D={D} ring={ring} by={by}: logit max err {err:.3e}")
    assert err <= OUT_TOL
    assert float((o["prob"] - torch.sigmoid(o["logit"])).abs().max()) == 0
    assert ("src_lead" in o) == (by == "neighbour")
    for side, ids in (("src", src), ("dst", dst)):
        sub = {k[len(side) + 1:]: v for k, v in o.items() if k.startswith(side + "_")}
        cnt = _check_rows(rig, ids, sub)
        eff, ev = o[f"{side}_effect"].double().cpu().numpy(), o[f"{side}_event"].cpu().numpy()
        worst = 0.0
        for p in range(P):
            assert not eff[p, cnt[p]:].any()
            ref = want[side][p]
            assert set(ev[p, :cnt[p]].tolist()) == set(ref)
            for j in range(cnt[p]):
                worst = max(worst, abs(eff[p, j] - ref[int(ev[p, j])]))
            if by == "neighbour":
                assert np.array_equal(o[f"{side}_lead"][p, :cnt[p]].cpu().numpy(), want["nodes"][int(ids[p])]["lead"])
                assert not bool(o[f"{side}_lead"][p, cnt[p]:].any())
        print(f"  {side} effects max err {worst:.3e}")
        assert worst <= EFF_TOL
        att = rig.eng.attention(ids)
        assert torch.equal(o[f"{side}_alpha"], att["alpha"].mean(-1))
    # z is embed()'s, bit for bit; loo_z against the oracle's masked forward; a second call gives the same bits
    nodes = o["nodes"].cpu().numpy()
    assert np.array_equal(nodes, _nodes(rig))
    assert torch.equal(_bits(o["z"]), _bits(rig.eng.embed(nodes)))
    lz, worst, singles = o["loo_z"].cpu(), 0.0, 0
    for r, v in enumerate(nodes):
        ref = want["nodes"][int(v)]
        c = ref["event"].size
        assert not bool(lz[r, c:].any())
        if c:
            worst = max(worst, float((lz[r, :c] - ref["loo_z"]).abs().max()))
        if c == 1:     # the only slot absent: the oracle's embedding of the node with an empty ring row
            singles += 1
            bare = copy.deepcopy(rig.lref)
            bare.e_id[int(v)] = -1
            empty = xr.oracle_embed(rig.ref, bare, rig.ev_t, rig.ev_msg, [int(v)])[0]
            assert float((lz[r, 0] - empty).abs().max()) <= TOL
    print(f"  loo_z max err {worst:.3e} ({singles} single-slot nodes)")
    assert worst <= TOL and singles > 0
    again = rig.eng.explain(src, dst, by=by)
    for k, v in o.items():
        assert torch.equal(_bits(again[k]), _bits(v)), k


@pytest.mark.parametrize("D,ring", CASES)
def test_one_call_equals_two_halves_bit_for_bit(D, ring):
    """Chunking and grid independence: a node's rows depend on neither the other nodes of the list nor the grid."""
    rig = _built(D, ring)
    eng, nodes = rig.eng, _nodes(rig)
    h = len(nodes) // 2
    for mode in (0, 1):
        whole = eng._explain_nodes(nodes, mode, True, True, "test")
        a, b = (eng._explain_nodes(x, mode, True, True, "test") for x in (nodes[:h], nodes[h:]))
        for k in ("z", "count", "event", "neighbour", "alpha", "loo_z"):
            assert torch.equal(_bits(whole[k]), _bits(torch.cat([a[k], b[k]]))), (mode, k)


def _state(eng):
    m, ld = eng.model, eng.loader
    return dict(memory=m.memory.memory, last_update=m.memory.last_update, store=m.store, node_gen=m.node_gen,
                neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t, flat=m.flat, grad=m.grad_flat, adam_m=eng.adam_m,
                adam_v=eng.adam_v, ctl=eng.ctl)


def test_attention_and_explain_change_nothing_and_eval_goes_on_unchanged():
    a, b = _rig(32, 10), _rig(32, 10)                                      # twins; b is never queried
    src, dst = xr.pairs(a.s)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _state(a.eng).items()}
    a.eng.attention(_nodes(a))
    a.eng.explain(src, dst)
    a.eng.explain(src, dst, by="neighbour")
    torch.cuda.synchronize()
    after = _state(a.eng)
    for k, v in before.items():
        if k == "ctl":
            keep = [i for i in range(24) if i != 3]                        # TGNX_CTL_GEN advances per C call
            assert torch.equal(after[k][keep], v[keep]), (after[k].tolist(), v.tolist())
            assert int(after[k][3]) - int(v[3]) == 3 and int(after[k][11]) == 0
        else:
            assert torch.equal(_bits(after[k]), _bits(v)), k
    sl = slice(xr.BATCHES * xr.B, (xr.BATCHES + 1) * xr.B)
    negs = torch.from_numpy(np.random.default_rng(11).choice(a.s.dst_nodes, size=(xr.B, xr.KN)))
    ra = a.eng.eval_batch(sl.start, xr.B, negs)
    rb = b.eng.eval_batch(sl.start, xr.B, negs)
    torch.cuda.synchronize()
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    for k in ("memory", "last_update", "store", "neighbors", "e_id", "t"):
        assert torch.equal(_bits(_state(a.eng)[k]), _bits(_state(b.eng)[k])), k


def test_invalid_ids():
    rig = _built(32, 10)
    eng, N = rig.eng, xr.N
    for bad in ([3, -1, 7], [N]):
        with pytest.raises(ValueError):
            eng.attention(bad)
        with pytest.raises(ValueError):
            eng.explain(bad, bad)
    ids = [3, -1, 7, N, 3]
    o = eng._explain_nodes(ids, 0, True, False, "test")
    torch.cuda.synchronize()
    assert int(o["n_invalid"]) == 2
    good = eng._explain_nodes([3, 7, 3], 0, True, True, "test")
    for k in ("z", "alpha", "loo_z"):
        assert not bool(o[k][[1, 3]].any()) and torch.equal(_bits(o[k][[0, 2, 4]]), _bits(good[k])), k
    assert not bool(o["count"][[1, 3]].any()) and torch.equal(o["count"][[0, 2, 4]], good["count"])
    for k in ("event", "neighbour"):
        assert bool((o[k][[1, 3]] == -1).all()) and torch.equal(o[k][[0, 2, 4]], good[k]), k
    att = eng.attention(ids, validate=False)
    assert int(att["n_invalid"]) == 2 and not bool(att["alpha"][[1, 3]].any()) and not bool(att["t"][[1, 3]].any())
    eng.check()


def test_two_hops_explain_is_refused_and_the_c_entry_launches_nothing():
    from tgnx import _lib
    rig = _built(32, 10, 2)
    eng = rig.eng
    src, dst = xr.pairs(rig.s)
    with pytest.raises(NotImplementedError):
        eng.explain(src, dst)
    n, K, D = 4, 10, 32
    nodes = torch.tensor([1, 2, 3, 4], device=DEV)
    z, cnt = torch.zeros(n, D, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    ev, nb = (torch.zeros(n, K, dtype=torch.long, device=DEV) for _ in range(2))
    al, loo = torch.zeros(n, K, 2, device=DEV), torch.full((n, K, D), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    gen0 = int(eng.ctl[3])
    b = eng._buffers(0)
    rc = _lib.lib().tgnx_tgn_explain(ctypes.byref(eng.cfg), ctypes.byref(b), p(nodes), n, 0, p(z), p(cnt), p(ev), p(nb),
                                     p(al), p(loo), None, eng._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"layers = 1" in _lib.lib().tgnx_last_error()      # TGNX_EINVAL
    assert int(eng.ctl[3]) == gen0 and bool((loo == 7.0).all())            # refused before any launch


def test_dropin_explain_flushes_once_and_explain_recommendations():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.data import SplitLoader, TemporalData
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    s, B, D = xr.stream(), xr.B, 32
    ref, _ = xr.new_oracle(D, 10)
    sd = ref.state_dict()
    data = TemporalData(src=torch.from_numpy(s.src), dst=torch.from_numpy(s.dst), t=torch.from_numpy(s.t),
                        msg=torch.from_numpy(s.msg))
    loader = SplitLoader(data, 0, 4 * B, B, np.zeros(4 * B, dtype=np.int64))

    def model_and_loader():
        m = TGNModel(xr.N, s.num_events, xr.MSG, D, DEV, ring=10, max_batch=B, max_neg=xr.KN, aggr="last", dropout=0.0)
        m.load_reference_state(sd)
        return m, LastNeighborLoader(xr.N, 10, device=DEV)

    model, nl = model_and_loader()
    with pytest.raises(RuntimeError, match="no engine"):
        tgn_epoch.explain(model, [1, 2], [3, 4])
    tgn_epoch.train(model, None, loader, nl, None, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train
    # the twin: an engine of its own in the same post-train state, flushed by hand
    m2, nl2 = model_and_loader()
    twin = TgnEngine(m2, nl2, dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), TgnAdam(m2, 1e-3),
                     dst_nodes=s.dst_nodes, seed=7)
    twin.reset_state()
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in _state(twin).items():
            if k not in ("grad", "adam_m", "adam_v"):
                v.copy_(_state(eng)[k])
    twin.flush()
    src, dst = torch.from_numpy(s.src[200:212].copy()), torch.from_numpy(s.dst[200:212].copy())
    want = twin.explain(src, dst, by="neighbour")
    got = pyg_epoch_utils.explain(model, src, dst, by="neighbour")
    assert not eng._mode_train                                             # switched to eval: flushed
    for k, v in want.items():
        assert torch.equal(_bits(got[k]), _bits(v)), k
    mem = model.memory.memory.clone()
    val, ids, pair, ex = pyg_epoch_utils.explain_recommendations(model, src[:5], 4, candidates=np.arange(3),
                                                                 exclude_self=True)
    assert torch.equal(model.memory.memory, mem)                           # no second flush, nothing written
    assert ids.shape == (5, 4) and bool((ids[:, 3] == -1).all())           # 3 candidates: the fourth slot is padding
    assert pair.size(0) == int((ids >= 0).sum()) and ex["logit"].numel() == pair.size(0)
    rows = twin.explain(src[:5].to(DEV)[pair[:, 0]], ids[pair[:, 0], pair[:, 1]])
    assert torch.equal(_bits(ex["logit"]), _bits(rows["logit"])) and torch.equal(_bits(ex["src_effect"]), _bits(rows["src_effect"]))
    assert float((torch.sigmoid(ex["logit"]) - val[pair[:, 0], pair[:, 1]]).abs().max()) <= 1e-6
