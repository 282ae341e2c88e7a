"""The TGN step against the oracle across memory widths D = 2 .. 128 (check_cfg accepts every even D in that range;
every other oracle comparison runs D = 32 or D = 100).  RefTGN ties the memory, time-encoding and embedding widths to
its one `hidden` value, so one sweep over D covers all three.

What branches on D in csrc/tgnx_tgn.hip, and the widths that reach each side:
  the predictor's LDS image of lin_src / lin_dst (tgn_pred_train): D % 8 == 4 stages unpadded rows with 16-byte
      LDS-DMA and contracts float4 columns (124: the largest, with a partial last wave); every other D takes pitch D + 1
      with element stores.  The 2-hop kernel stages 192 x 16 float4 per round: D <= 110 is one round, 112 .. 128 two;
  the 1-hop train attention: paired channels need C = D / 2 even; C odd (2, 6, 66, 126) runs attn_centre per root;
  the GEMM operand loaders' vec4(): D = 2 mod 4 leaves every row of memory, P, Z and the weights 8-byte aligned only;
  the predictor's two lane rounds o = lane + 64 q < D: 64 leaves the second empty, 66 gives it 2 lanes, 128 fills it;
  its backward split ow = ceil(D / NW) <= OL: equality at 128, ow = 1 with idle waves at 2;
  the launch's dynamic LDS 2 D (D + 1) 4 bytes: 132,096 at 128, 48 at 2 (the marking / plan terms then set it);
  C = 1 (D = 2): a one-channel head, sqrt(C) = 1, a 6-wide GRU gate block.

  1  train steps, flush, eval    Rig(N = 300, B = 50, nb = 6, seed 3, ring 10), dropout off: 5 compared train steps with
     injected negatives, then flush and one eval batch with 20 negatives, at tgn_oracle_steps.py's bounds (outputs and
     eval scores 2e-5, loss 1e-5 relative, memory 1e-5, every gradient tensor 2e-3 relative L2, parameters after Adam,
     last_update and the ring exact).  Asserted so that a case cannot pass without running its branch: which side of
     each D-dependent branch the case takes (plain arithmetic against the table's literals), and from the oracle's
     loader that the roots of each of steps 2 .. 4 include an empty ring row, a partly filled one and a full one.
  2  the bench's step forms      test_gpu_tgn.py's pipelined / parity-set against resident comparison (graph replay,
     device negatives, dropout 0.1, a partial last batch, a step past the split) at the edge widths: the marking and
     plan blocks share the launch's dynamic LDS with the image, which D = 6 makes the smallest term and D = 128 132 KB.
  3  read-only and ingest calls  on section 1's state, D in {6, 128} x layers in {1, 2}: embed() of the query test's
     120 nodes against the oracle's eval forward and score() against the oracle's predictor on those embeddings (2e-5
     in the `_close` metric); observe() on a twin against eval_batch on the other, state bit for bit.
  4  widths outside the domain   0, 7, 130, -2 raise check_cfg's message and leave a later valid model clean (the
     host-only half is tests/test_cabi.py::test_tgn_param_layout_refuses_widths_outside_the_domain)."""
import numpy as np
import pytest
import torch

from tgn_oracle_steps import Rig

pytestmark = pytest.mark.gpu

N, B, STEPS = 300, 50, 5
PRED2_ROUND = 192 * 16      # float4 per matrix the 2-hop predictor stages in one round (NST x PRED_SU)

# (D, d, layers, aggr, updater, emb), then what the case's numbers must select:
# flat image (D % 8 == 4), C odd, second staging round (2 hops)
CASES = [
    ((2, 16, 1, "last", "gru", (0, 0)), (False, True, False)),      # C = 1, ow = 1, the 48 B image
    ((6, 16, 1, "last", "gru", (0, 0)), (False, True, False)),      # unpaired attention, D = 2 mod 4 loaders
    ((64, 16, 1, "last", "gru", (0, 0)), (False, False, False)),    # second lane round empty, padded image
    ((66, 16, 1, "last", "gru", (0, 0)), (False, True, False)),     # second lane round with 2 lanes, C odd
    ((124, 16, 1, "last", "gru", (0, 0)), (True, False, False)),    # largest flat image: DMA staging, partial last wave
    ((126, 16, 1, "last", "gru", (0, 0)), (False, True, False)),    # largest C odd (63)
    ((128, 16, 1, "last", "gru", (0, 0)), (False, False, False)),   # the cap: C = 64, 132 KB LDS, ow == OL
    ((128, 172, 1, "last", "gru", (0, 0)), (False, False, False)),  # widest message row, Qm = 556
    ((2, 16, 2, "last", "gru", (0, 0)), (False, True, False)),      # non-ATT predictor, smallest
    ((6, 16, 2, "last", "gru", (0, 0)), (False, True, False)),      # 2-hop, C odd
    ((66, 16, 2, "last", "gru", (0, 0)), (False, True, False)),     # 2-hop, second lane round with 2 lanes
    ((110, 16, 2, "last", "gru", (0, 0)), (False, True, False)),    # last width staged in one round
    ((112, 16, 2, "last", "gru", (0, 0)), (False, False, True)),    # first width that needs the second staging round
    ((128, 16, 2, "last", "gru", (0, 0)), (False, False, True)),    # second round, full
    ((2, 16, 2, "mean", "gru", (0, 0)), (False, True, False)),      # mean aggregation at C = 1
    ((126, 5, 1, "mean", "gru", (0, 0)), (False, True, False)),     # D and d both unaligned
    ((128, 5, 1, "mean", "rnn", (0, 1)), (False, False, False)),    # Qm unaligned; DyRep embedding messages at the cap
    ((6, 16, 1, "last", "rnn", (1, 1)), (False, True, False)),      # DyRep embeddings at C odd (the Zc scalar stores)
    ((2, 5, 1, "last", "rnn", (0, 0)), (False, True, False)),       # RNNCell at the minimum
]
SHARED = [(6, 1), (128, 1), (6, 2), (128, 2)]    # (D, layers) of the d = 16 last / gru cases section 3 goes on from


def _id(case):
    D, d, layers, aggr, updater, emb = case
    return f"D{D}-d{d}-L{layers}-{aggr}-{updater}-emb{emb[0]}{emb[1]}"


def _steps_flush_eval(case):
    """Section 1 for one case; returns the rig in the state after the eval batch."""
    D, d, layers, aggr, updater, emb = case
    rig = Rig(aggr=aggr, N=N, B=B, d=d, D=D, nb=STEPS + 1, seed=3, ring=10, layers=layers, updater=updater, emb=emb)
    rng = np.random.default_rng(1)
    for st in range(STEPS):
        _, src, pos = rig.batch(st)
        neg = torch.from_numpy(rng.choice(rig.s.dst_nodes, size=B))
        if st >= 2:     # the ring rows this step's attention reads: empty, partly filled and full roots
            roots = torch.cat([src, pos, neg]).unique().numpy()
            fills = np.bincount((rig.lref.e_id[roots] >= 0).sum(1), minlength=11)
            print(f"step {st}: root fills {fills}")
            assert fills[0] > 0 and fills[1:10].sum() > 0 and fills[10] > 0, (st, fills)
        rig.train_step(st, neg)
    negs = torch.from_numpy(rng.choice(rig.s.dst_nodes, size=(B, 20)))
    rig.flush_and_eval(STEPS, negs)
    print("worst:", {k: f"{v:.3e}" for k, v in rig.worst.items()})
    return rig


_RIGS = {}


def _shared_rig(D, layers):
    """The (D, 16, layers, last, gru) case's rig after section 1, built once."""
    if (D, layers) not in _RIGS:
        _RIGS[(D, layers)] = _steps_flush_eval((D, 16, layers, "last", "gru", (0, 0)))
    return _RIGS[(D, layers)]


@pytest.mark.parametrize("case,branch", CASES, ids=[_id(c) for c, _ in CASES])
def test_tgn_mem_dim_matches_oracle(case, branch):
    """Measured on an MI355X, worst over the 19 cases: train outputs 1.2e-7 and eval scores 1.2e-7 (bound 2e-5), loss
    1.7e-7 relative (1e-5), memory 6.8e-7 (1e-5; D = 128, d = 5, mean / rnn with embedding messages), gradients 1.8e-5
    relative L2 (2e-3; D = 2, d = 5, rnn, where some attention gradients have norms near 1e-5 — every other case stays
    at or below 2.4e-6).  With the 2-hop staging loop cut to its first round in a scratch build (part of the LDS image
    left unwritten) the 2-hop cases D = 112 and D = 128 fail and D = 110 passes."""
    D, d, layers, aggr, updater, emb = case
    flat, c_odd, second_round = branch
    assert D % 2 == 0 and 2 <= D <= 128
    assert (D % 8 == 4) == flat, D
    assert ((D // 2) % 2 == 1) == c_odd, D
    assert (layers == 2 and D * D // 4 > PRED2_ROUND) == second_round, D
    if (D, layers) in SHARED and (d, aggr, updater, emb) == (16, "last", "gru", (0, 0)):
        _shared_rig(D, layers)      # (section 3 goes on from this state)
    else:
        _steps_flush_eval(case)


# ------------------------------------------------------------------ 2: the bench's step forms
@pytest.mark.parametrize("pp,table", [(True, True), (False, False)])
@pytest.mark.parametrize("layers,D", [(1, 6), (1, 128), (2, 6), (2, 112)])
def test_tgn_pipelined_equals_resident_at_edge_widths(layers, D, pp, table):
    """test_gpu_tgn.py::test_tgn_pipelined_equals_resident's comparison, its asserts and tolerances, at other widths."""
    from test_gpu_tgn import pipelined_equals_resident
    pipelined_equals_resident(layers, "gru", (0, 0), pp, table, D=D)


# ------------------------------------------------------------------ 3: read-only and ingest calls
def _query():
    from test_gpu_tgn_query import _close, _query_nodes
    return _close, _query_nodes


@pytest.mark.parametrize("D,layers", SHARED)
def test_embed_and_score_match_oracle(D, layers):
    """embed() against the oracle's eval forward and score() against its predictor on those embeddings, after the
    case's train steps, flush and eval batch (all 300 events are in the rings).  Measured on an MI355X, worst over the four cases: embeddings
    7.2e-7 at scale 1.9 (bound 3.8e-5), scores 6.0e-8 (2e-5)."""
    _close, _query_nodes = _query()
    rig = _shared_rig(D, layers)
    eng, s = rig.eng, rig.s
    nodes, hub, empty = _query_nodes(s, (STEPS + 1) * B)
    assert nodes.size == 120
    assert int((eng.loader.e_id[empty] >= 0).sum()) == 0 and int((eng.loader.e_id[hub] >= 0).sum()) == 10
    z = eng.embed(nodes)
    assert z.shape == (120, D) and z.dtype == torch.float32
    want = rig.oracle_embed(nodes)
    _close(z, want, 2e-5)
    assert torch.equal(z[0], z[2]) and torch.equal(z[1], z[117])          # duplicates: the same row
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, 120, 40), rng.integers(0, 120, 40)        # pairs out of the query set
    dst[:3] = src[:3]
    p = eng.score(nodes[src], nodes[dst])
    assert p.shape == (40,)
    with torch.no_grad():
        _close(p, rig.ref.link_pred(want[src], want[dst]).view(-1), 2e-5)   # (RefLinkPredictor returns the sigmoid)
    eng.check()


STATE = ("memory", "last_update", "store", "node_gen", "neighbors", "e_id", "t")
CTL = {"BATCH_START": 0, "CUR_EID": 1, "B": 2, "GEN": 3, "NB": 10, "ERR": 11}


def _state(eng):
    m, ld = eng.model, eng.loader
    return dict(memory=m.memory.memory, last_update=m.memory.last_update, store=m.store, node_gen=m.node_gen,
                neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t, ctl=eng.ctl)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _twin(rig, D, layers):
    """A fresh engine over the rig's stream with the rig's (trained) parameters, reset and flushed."""
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    s, dev = rig.s, torch.device("cuda")
    model = TGNModel(N, s.num_events, 16, D, dev, ring=10, max_batch=B, max_neg=20, aggr="last", dropout=0.0,
                     layers=layers)
    with torch.no_grad():
        model.flat.copy_(rig.model.flat)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=dev),
                    dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), TgnAdam(model, 1e-3),
                    dst_nodes=s.dst_nodes, seed=0)
    eng.reset_state()
    eng.flush()
    return eng


@pytest.mark.parametrize("D,layers", SHARED)
def test_observe_equals_the_eval_step(D, layers):
    """Twin engines with the case's trained parameters, 4 eval batches each; then eval_batch against observe on batch 4:
    memory, last_update, stores, node_gen and the ring bit for bit, the ctl words equal; then batch 5 scores equal."""
    rig = _shared_rig(D, layers)
    a, b = _twin(rig, D, layers), _twin(rig, D, layers)
    negs = torch.from_numpy(np.random.default_rng(9).choice(rig.s.dst_nodes, size=((STEPS + 1) * B, 20)))
    for st in range(4):
        for e in (a, b):
            e.eval_batch(st * B, B, negs[st * B:(st + 1) * B])
    a.eval_batch(4 * B, B, negs[4 * B:5 * B])
    b.observe(4 * B, B)
    torch.cuda.synchronize()
    a.check()
    b.check()
    sa, sb = _state(a), _state(b)
    assert float(sa["memory"].abs().max()) > 0 and int((sa["e_id"] >= 0).sum()) > 0
    for k in STATE:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), k
    for name, i in CTL.items():
        assert int(sa["ctl"][i]) == int(sb["ctl"][i]), (name, sa["ctl"].tolist(), sb["ctl"].tolist())
    assert int(sa["ctl"][CTL["ERR"]]) == 0
    ra = a.eval_batch(5 * B, B, negs[5 * B:])
    rb = b.eval_batch(5 * B, B, negs[5 * B:])
    torch.cuda.synchronize()
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    a.check()
    b.check()


# ------------------------------------------------------------------ 4: widths outside the domain
def test_widths_outside_the_domain_are_refused():
    from tgnx.tgn import TGNModel
    for D in (0, 7, 130, -2):
        with pytest.raises(RuntimeError, match="mem_dim must be even and <= 128"):
            TGNModel(N, 100, 16, D, torch.device("cuda"), ring=10, max_batch=B, max_neg=1, dropout=0.0)
    rig = Rig(N=N, B=B, d=16, D=2, nb=2, seed=3)      # a later valid model: its step ends without an error flag
    neg = torch.from_numpy(np.random.default_rng(1).choice(rig.s.dst_nodes, size=B))
    rig.train_step(0, neg)
    assert int(rig.eng.ctl[CTL["ERR"]]) == 0
