"""GPU tests of a node space that grows: tgnx_tgn_grow_nodes / tgnx_tgn_grow_store, TgnEngine.grow_nodes /
reserve_nodes / node_capacity, observe_events(grow=True) / append_events_grow, load_stream_state_grow,
LastNeighborLoader.grow, TGNModel.grow_nodes and the drop-in grow_nodes / observe_grow.

Setup: the small stream of test_gpu_tgn_observe.py — 600 wiki-shaped events over 300 nodes (msg_dim 16, D = 32, ring
10, B = 50), parameters from a RefTGN state dict, dropout 0 — with its nodes relabelled by order of first appearance,
so that new ids arrive through the whole stream.  N0 = the distinct nodes of rows [0, 300) (computed here: 70 of the 93
the stream touches).  The small engine is built at N0 over the first 300 rows, the twin at 300 nodes over the same
rows; both are reset and take the same calls.  Engines have no dst_nodes (every default that means "all nodes" follows
cfg.num_nodes) except in the train tests, where the negative pool must not depend on N.

Where flush() stands.  flush() is the reference's train(False): _update_memory(arange(N)) runs the updater on EVERY
row, so a node without a stored message goes from memory h to cell(0, h) — on a fresh engine from 0 to one constant
nonzero row.  A twin flushed while it has rows the small engine lacks therefore holds that row where grow_nodes
leaves the contract's memory 0, and the two differ from the first update of such a node on.  That is the reference's
flush, not the growth; the twin rule is stated for flushes made while both engines have the same node count.  So the
engines here are reset, not flushed, before the growth point, `test_flush_and_the_twin_rule` flushes both after it
(equal) and pins the exception (a twin flushed before it differs in exactly the rows the small engine lacked).

THE TWIN RULE: an engine built at N0 and grown to N1 at any point equals, from then on, an engine built at N1 and fed
the same calls — every stream_state() tensor torch.equal, the WHOLE ctl block included (the grow path does not
advance GEN: new rows carry node_gen 0, which no generation equals once a step has run), and embed / recommend /
recommend_filtered / rank / eval_batch outputs equal.  Observe and eval are deterministic, so this is equality.  Train
steps after a growth: memory within 1e-4 and parameters within 2e-5 (the run-to-run bounds of the step's float atomics
that test_gpu_tgn_observe.py uses), ring, stores and last_update exact.

  twin, explicit   observe [0, 300) on both, grow_nodes(300) once, append the other 300 rows, observe [300, 550), queries,
                   eval_batch on [550, 600) with 5 negatives from [0, 300); six model forms;
  twin, automatic  rows [300, 600) through observe_events(grow=True, batch=50) in chunks of 50, 1, 137, 112 against
                   observe_range per chunk: num_nodes ends at the largest id + 1, node_capacity follows
                   grown_node_capacity through two reallocations, the twin's other rows are reset rows;
  pad reference    stream_state() before grow_nodes(N1), padded by grow_ref.pad_state, equals stream_state() after;
  oracle           1 hop / last: every batch through RefTGN built at 300 nodes (memory within 2e-5, the rest exact);
  edges            by one node, across multiples of 64 and 256, N0 = 1, 40 -> 41 with max_batch 32 (N < 2B on both
                   sides), ring 4, an engine that never observed, two growths in a row, around compact_events,
                   ensure_neg(999) after, n <= N, refused appends, clamped ids, null pointers to the C call;
  bindings         a bound resident eval pass is re-bound by grow_nodes and goes on (cursor and reciprocal ranks kept);
                   a captured train graph is dropped and the next resident steps match the twin; _prefetched is cleared;
  checkpoints      grown -> fresh 300-node engine (strict load), -> fresh N0 engine (load_stream_state_grow only),
                   and a state saved at N0 -> 300-node engine (rows beyond are reset rows);
  drop-in          pyg_epoch_utils.observe_grow after train() equals a hand-grown twin; a model and loader grown on
                   their own (no engine) equal fresh ones."""
import ctypes
import types

import numpy as np
import pytest
import torch

from grow_ref import crop_state, is_reset_rows, pad_state, same_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N1, d, D, B, KN, NEV, HALF = 300, 16, 32, 50, 5, 600, 300
TOL = 2e-5
FORMS = {"1hop_last": dict(layers=1, aggr="last"), "1hop_mean": dict(layers=1, aggr="mean"),
         "2hop_last": dict(layers=2, aggr="last"), "2hop_mean": dict(layers=2, aggr="mean"),
         "rnn": dict(layers=1, aggr="last", updater="rnn"),
         "dyrep_emb": dict(layers=1, aggr="last", memory="dyrep", use_src_emb_in_msg=True)}
CHUNKS = (50, 1, 137, 112)
GEN, ERR = 3, 11


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _relabel(src, dst):
    """Node ids by order of first appearance in the interleaved (src, dst) rows."""
    ids = np.stack([src, dst], 1).reshape(-1)
    _, first = np.unique(ids, return_index=True)
    order = ids[np.sort(first)]
    rel = np.full(int(ids.max()) + 1, -1, dtype=np.int64)
    rel[order] = np.arange(order.size)
    return rel[src], rel[dst]


_STREAM = {}


def _stream(num_events=NEV, num_nodes=N1):
    """(events dict of numpy arrays, first row that names node id >= n for every n) of the relabelled stream."""
    key = (num_events, num_nodes)
    if key not in _STREAM:
        from tgnx.synth import make_stream
        s = make_stream("tgbl-wiki", seed=5, num_events=num_events, num_nodes=num_nodes, msg_dim=d)
        src, dst = _relabel(s.src, s.dst)
        ev = dict(src=src, dst=dst, t=s.t.astype(np.float32), msg=s.msg)
        _STREAM[key] = ev
    return _STREAM[key]


def _rows(ev, lo, hi):
    return {k: v[lo:hi] for k, v in ev.items()}


def _nodes_in(ev, lo, hi):
    return int(max(ev["src"][lo:hi].max(), ev["dst"][lo:hi].max())) + 1


def _n0():
    return _nodes_in(_stream(), 0, HALF)


_SD = {}


def _sd(form):
    if form not in _SD:
        from oracle.tgn_ref import RefTGN
        kw = dict(FORMS[form])
        kw.pop("memory", None)
        torch.manual_seed(0)
        _SD[form] = RefTGN(N1, d, hidden=D, dropout=0.0, **kw).state_dict()
    return _SD[form]


def _engine(n_nodes, events, form="1hop_last", ring=10, max_batch=B, dst_nodes=None):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    rows = int(events["src"].shape[0])
    model = TGNModel(n_nodes, rows, d, D, DEV, ring=ring, max_batch=max_batch, max_neg=KN, dropout=0.0, **FORMS[form])
    model.load_reference_state(_sd(form))
    eng = TgnEngine(model, LastNeighborLoader(n_nodes, ring, device=DEV), events, TgnAdam(model, 1e-3),
                    dst_nodes=dst_nodes, seed=7)
    eng.reset_state()
    return eng


def _cpu(state):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state.items()}


def _assert_twins(a, b, skip_ctl=()):
    torch.cuda.synchronize()
    a.check()
    b.check()
    sa, sb = _cpu(a.stream_state()), _cpu(b.stream_state())
    diff = same_state(sa, sb, skip_ctl) + same_state(sb, sa, skip_ctl)
    assert diff == [], (diff, sa["ctl"].tolist(), sb["ctl"].tolist())
    assert int(sa["ctl"][ERR]) == 0
    assert torch.equal(a.model.flat, b.model.flat)                       # no parameter moved
    return sa


def _bufs(e):
    m, ld = e.model, e.loader
    return (m.memory.memory, m.memory.last_update, m.node_gen, m.store, ld.neighbors, ld.e_id, ld.t, ld._assoc, e.ws)


def _ptrs(e):
    return tuple(x.data_ptr() for x in _bufs(e))


def _pair(ev, n0, n1, split, **kw):
    """(small engine at n0, twin at n1), both over rows [0, split) of ev."""
    assert _nodes_in(ev, 0, split) <= n0
    return _engine(n0, _rows(ev, 0, split), **kw), _engine(n1, _rows(ev, 0, split), **kw)


def _feed(engines, ev, lo, hi, batch=B):
    """Rows [lo, hi) of ev whose ids fit the engines, appended and observed on each."""
    n = int(engines[0].cfg.num_nodes)
    keep = (ev["src"][lo:hi] < n) & (ev["dst"][lo:hi] < n)
    rows = {k: v[lo:hi][keep] for k, v in ev.items()}
    for e in engines:
        assert int(e.cfg.num_nodes) == n
        e.observe_events(rows["src"], rows["dst"], rows["t"], rows["msg"], batch=batch)
    return int(keep.sum())


def _query_nodes(n0, n1):
    rnd = np.random.default_rng(3).integers(0, n1, 113)
    return np.concatenate([[0, n0 - 1, n0, min(n0 + 1, n1 - 1), n1 - 1, 0, n0], rnd]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ twin, explicit
@pytest.mark.parametrize("form", list(FORMS))
def test_twin_explicit(form):
    ev, n0 = _stream(), _n0()
    assert 1 < n0 < _nodes_in(ev, 0, NEV) <= N1
    small, twin = _pair(ev, n0, N1, HALF, form=form)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    gen = int(small.ctl[GEN])
    assert small.grow_nodes(N1) == N1 and int(small.cfg.num_nodes) == small.model.num_nodes == small.loader.num_nodes == N1
    assert small.node_capacity == N1 and int(small.ctl[GEN]) == gen
    _assert_twins(small, twin)                                            # equal straight after the growth
    rest = _rows(ev, HALF, NEV)
    for e in (small, twin):
        assert e.append_events(rest["src"], rest["dst"], rest["t"], rest["msg"]) == (HALF, NEV - HALF)
        e.observe_range(HALF, NEV - B, B)
    _assert_twins(small, twin)
    nodes = _query_nodes(n0, N1)
    assert nodes.size == 120 and nodes.min() == 0 and nodes.max() == N1 - 1
    assert torch.equal(small.embed(nodes), twin.embed(nodes))
    src = torch.from_numpy(ev["src"][NEV - B:NEV - B + 7].copy())
    dst = torch.from_numpy(ev["dst"][NEV - B:NEV - B + 7].copy())
    for a, b in zip(small.recommend(src, 10), twin.recommend(src, 10)):               # over all 300 nodes
        assert torch.equal(a, b) and a.shape == (7, 10)
    for a, b in zip(small.recommend_filtered(src, 10, exclude_seen=True), twin.recommend_filtered(src, 10, exclude_seen=True)):
        assert torch.equal(a, b)
    ra, rb = small.rank(src, dst), twin.rank(src, dst)
    assert all(torch.equal(a, b) for a, b in zip(ra, rb)) and ra[0].shape == (7,) and int(ra[3].max()) > _n0()
    negs = torch.from_numpy(np.random.default_rng(9).integers(0, N1, size=(B, KN)))
    outs = []
    for e in (small, twin):
        p, n, r = e.eval_batch(NEV - B, B, negs)
        outs.append((p.clone(), n.clone(), r.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    _assert_twins(small, twin)


# ------------------------------------------------------------------------------------------------ twin, automatic
def test_twin_automatic():
    from tgnx.tgn import grown_node_capacity
    ev, n0 = _stream(), _n0()
    small = _engine(n0, _rows(ev, 0, HALF))
    twin = _engine(N1, ev)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    want_cap, caps, nodes, lo = n0, [small.node_capacity], [n0], HALF
    assert caps == [n0]
    for n in CHUNKS:
        r = _rows(ev, lo, lo + n)
        assert small.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B, grow=True) == (lo, n)
        twin.observe_range(lo, lo + n, B)                                 # the same per-call batches
        lo += n
        need = max(nodes[-1], _nodes_in(ev, lo - n, lo))
        want_cap = grown_node_capacity(want_cap, need)
        nodes.append(need)
        caps.append(small.node_capacity)
        assert int(small.cfg.num_nodes) == need and small.node_capacity == want_cap
    n_end = _nodes_in(ev, 0, NEV)
    assert int(small.cfg.num_nodes) == small.loader.num_nodes == small.model.num_nodes == n_end < N1
    assert len(set(caps)) - 1 >= 2, caps                                  # at least two reallocations
    assert len(set(nodes)) - 1 > len(set(caps)) - 1                       # and a growth inside the capacity
    torch.cuda.synchronize()
    small.check()
    twin.check()
    got = _cpu(small.stream_state())
    want, rest = crop_state(_cpu(twin.stream_state()), n_end)
    assert got["memory"].shape[0] == n_end and same_state(got, want) == [] and same_state(want, got) == []
    assert is_reset_rows(rest)                                            # capacity rows never leak, the twin's are untouched
    q = np.arange(n_end)
    assert torch.equal(small.embed(q), twin.embed(q))


# ------------------------------------------------------------------------------------------------ pad reference, edges
@pytest.mark.parametrize("ring,grow_by", [(10, 1), (10, 128 - 70), (10, 257 - 70), (4, 1), (4, 300 - 70)])
def test_growth_equals_the_pad_reference_and_the_twin(ring, grow_by):
    """By one node, across 128 = 2 x 64 (a bitmap word), across 256 (a workgroup), ring 4 and ring 10: the state after
    grow_nodes is the padded state before it, and the stream goes on as on a twin built at n1."""
    ev, n0 = _stream(), _n0()
    n1 = n0 + grow_by
    small, twin = _pair(ev, n0, n1, HALF, ring=ring)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    before = _cpu(small.stream_state())
    assert small.grow_nodes(n1) == n1
    after = _cpu(small.stream_state())
    want = pad_state(before, n1)
    assert same_state(want, after) == [] and same_state(after, want) == []           # every ctl word included
    assert int(after["num_nodes"]) == n1 and after["neighbors"].shape == (n1, ring)
    fed = _feed((small, twin), ev, HALF, NEV)
    assert fed > 0 and (grow_by > 1 or fed < NEV - HALF)
    sa = _assert_twins(small, twin)
    assert int((sa["last_update"][n0:] > 0).sum()) > 0 or grow_by == 1               # the new nodes were used
    q = np.arange(n1)
    assert torch.equal(small.embed(q), twin.embed(q))


def test_one_node_graph():
    """N0 = 1: 40 self-loops on node 0, then five nodes."""
    rng = np.random.default_rng(1)
    n = 120
    src, dst = rng.integers(0, 5, n), rng.integers(0, 5, n)
    src[:40] = dst[:40] = 0
    ev = dict(src=src, dst=dst, t=np.sort(rng.random(n) * 1000).astype(np.float32),
              msg=rng.standard_normal((n, d)).astype(np.float32))
    small, twin = _pair(ev, 1, 5, 40, max_batch=16)
    for e in (small, twin):
        e.observe_range(0, 40, 16)
    before = _cpu(small.stream_state())
    assert small.grow_nodes(5) == 5
    assert same_state(pad_state(before, 5), _cpu(small.stream_state())) == []
    assert _feed((small, twin), ev, 40, n, batch=16) == n - 40
    _assert_twins(small, twin)
    assert torch.equal(small.embed(np.arange(5)), twin.embed(np.arange(5)))


@pytest.mark.parametrize("form", ["dyrep_emb", "2hop_last"])
def test_tiny_graph_below_two_batches(form):
    """40 -> 41 nodes with max_batch = 32: N < 2B on both sides of the growth (the root capacity is N)."""
    rng = np.random.default_rng(4)
    n = 200                                              # uniform endpoints over 41 nodes: all appear, node 40 at row 69
    src, dst = _relabel(rng.integers(0, 41, n), rng.integers(0, 41, n))
    ev = dict(src=src, dst=dst, t=np.sort(rng.random(n) * 1000).astype(np.float32),
              msg=rng.standard_normal((n, d)).astype(np.float32))
    assert _nodes_in(ev, 0, n) == 41
    split = int(np.argmax(np.maximum(ev["src"], ev["dst"]) >= 40))       # the first row naming node 40
    assert 32 < split < n - 64
    small, twin = _pair(ev, 40, 41, split, form=form, max_batch=32)
    for e in (small, twin):
        e.observe_range(0, split, 32)
    assert small.grow_nodes(41) == 41 and 41 < 2 * 32
    assert _feed((small, twin), ev, split, n, batch=32) == n - split
    assert int(small.model.memory.last_update[40]) > 0
    _assert_twins(small, twin)
    assert torch.equal(small.embed(np.arange(41)), twin.embed(np.arange(41)))


def test_never_observed_and_two_growths_in_a_row():
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)
    held, p0 = _bufs(small), _ptrs(small)    # (the first allocations stay alive: the allocator may otherwise hand their
                                             # addresses, free after the first growth, to the second growth's tensors)
    assert small.grow_nodes(n0 + 7) == n0 + 7                             # nothing observed yet
    assert small.grow_nodes(N1) == N1                                     # and again, no call between
    assert all(a != b for a, b in zip(_ptrs(small), p0))
    del held
    _assert_twins(small, twin)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    assert _feed((small, twin), ev, HALF, NEV) == NEV - HALF
    _assert_twins(small, twin)


@pytest.mark.parametrize("grow_first", [False, True])
def test_growth_around_compaction(grow_first):
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    if grow_first:
        small.grow_nodes(N1)
    ka, kb = small.compact_events(), twin.compact_events()
    assert torch.equal(ka, kb) and 0 < ka.numel() < HALF
    if not grow_first:
        small.grow_nodes(N1)
    _assert_twins(small, twin)
    assert small.model.store.numel() == 4 * N1 + 2 * small.event_capacity
    assert _feed((small, twin), ev, HALF, NEV) == NEV - HALF
    _assert_twins(small, twin)
    ka, kb = small.compact_events(), twin.compact_events()
    assert torch.equal(ka, kb)
    _assert_twins(small, twin)


def test_ensure_neg_after_growth_and_noop_and_refusals():
    from tgnx import _lib
    from tgnx.tgn import TgnGrowOut
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    torch.cuda.synchronize()
    # n <= N: nothing changes, not even an allocation
    before, p0 = _cpu(small.stream_state()), _ptrs(small)
    for n in (n0, n0 - 1, 1, 0, -3):
        assert small.grow_nodes(n) == n0
    small.reserve_nodes(n0)
    assert _ptrs(small) == p0 and small.node_capacity == n0 and same_state(before, _cpu(small.stream_state())) == []
    # id N without grow: refused, the engine untouched
    r = {k: np.array(v, copy=True) for k, v in _rows(ev, HALF, HALF + 40).items()}
    r["src"][:] = np.minimum(r["src"], n0 - 1)
    r["dst"][:] = np.minimum(r["dst"], n0 - 1)
    r["dst"][17] = n0
    with pytest.raises(ValueError, match="node ids"):
        small.append_events(r["src"], r["dst"], r["t"], r["msg"])
    with pytest.raises(ValueError, match="node ids"):
        small.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B)
    with pytest.raises(ValueError, match="validate"):
        small.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B, validate=False, grow=True)
    neg = {k: np.array(v, copy=True) for k, v in r.items()}
    neg["src"][3] = -1
    with pytest.raises(ValueError, match="negative"):
        small.append_events_grow(neg["src"], neg["dst"], neg["t"], neg["msg"])
    with pytest.raises(ValueError, match="2\\^31"):
        small.grow_nodes(1 << 31)
    big = {k: np.array(v, copy=True) for k, v in r.items()}
    big["dst"][17] = (1 << 31) + 5
    with pytest.raises(ValueError):
        small.append_events_grow(big["src"], big["dst"], big["t"], big["msg"])
    torch.cuda.synchronize()
    assert _ptrs(small) == p0 and small.num_events == HALF and int(small.cfg.num_nodes) == n0
    assert same_state(before, _cpu(small.stream_state())) == []
    # null pointers to the C call: TGNX_EINVAL, nothing launched
    L = _lib.lib()
    b, out = small._buffers(0), TgnGrowOut()
    bad = torch.zeros(1, dtype=torch.long, device=DEV)
    spare = torch.zeros(4 * N1 + 2 * HALF, dtype=torch.long, device=DEV)
    out.store = spare.data_ptr()
    for args in ((None, ctypes.byref(b), N1, N1, ctypes.byref(out), bad.data_ptr()),
                 (ctypes.byref(small.cfg), None, N1, N1, ctypes.byref(out), bad.data_ptr()),
                 (ctypes.byref(small.cfg), ctypes.byref(b), N1, N1, None, bad.data_ptr()),
                 (ctypes.byref(small.cfg), ctypes.byref(b), N1, N1, ctypes.byref(out), None),
                 (ctypes.byref(small.cfg), ctypes.byref(b), n0 - 1, N1, ctypes.byref(out), bad.data_ptr())):
        assert L.tgnx_tgn_grow_nodes(*args, small._stream()) == -1 and len(L.tgnx_last_error()) > 0
    assert L.tgnx_tgn_grow_nodes(ctypes.byref(small.cfg), ctypes.byref(b), N1, N1, ctypes.byref(out), bad.data_ptr(),
                                 small._stream()) == -1                    # (nbr has no new allocation)
    assert L.tgnx_tgn_grow_store(ctypes.byref(small.cfg), ctypes.byref(b), N1, None, bad.data_ptr(), small._stream()) == -1
    torch.cuda.synchronize()
    assert int(spare.abs().sum()) == 0 and same_state(before, _cpu(small.stream_state())) == []
    # unvalidated ids are still clamped, against the grown N
    small.grow_nodes(N1)
    clamp = {k: np.array(v, copy=True) for k, v in r.items()}
    clamp["src"][3], clamp["dst"][4] = -7, N1 + 5
    for e in (small, twin):
        assert e.append_events(clamp["src"], clamp["dst"], clamp["t"], clamp["msg"], validate=False) == (HALF, 40)
        assert int(e.src[HALF + 3]) == 0 and int(e.dst[HALF + 4]) == N1 - 1
        e.observe_range(HALF, HALF + 40, B)
    _assert_twins(small, twin)
    # ensure_neg after a growth: the workspace is sized from the grown config
    negs = torch.from_numpy(np.random.default_rng(2).integers(0, N1, size=(40, 999)))
    outs = []
    for e in (small, twin):
        e.ensure_neg(999)
        assert int(e.cfg.max_neg) == 999
        p, n, rr = e.eval_batch(HALF, 40, negs)
        outs.append((p.clone(), n.clone(), rr.clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    _assert_twins(small, twin)


def test_flush_and_the_twin_rule():
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    small.grow_nodes(N1)
    for e in (small, twin):
        e.flush()                                                         # same node count on both: the rule holds
    sa = _assert_twins(small, twin)
    assert bool(sa["memory"][N1 - 1].any()) and not sa["store_nodes"][:, [1, 3]].any()
    assert _feed((small, twin), ev, HALF, NEV) == NEV - HALF
    _assert_twins(small, twin)
    # the exception: a twin flushed while it had rows the small engine lacked holds cell(0, 0) there
    small, twin = _pair(ev, n0, N1, HALF)
    for e in (small, twin):
        e.flush()
        e.observe_range(0, HALF, B)
    small.grow_nodes(N1)
    torch.cuda.synchronize()
    sa, sb = _cpu(small.stream_state()), _cpu(twin.stream_state())
    assert same_state(sa, sb) == ["memory"]
    assert torch.equal(sa["memory"][:n0], sb["memory"][:n0]) and not sa["memory"][n0:].any()
    assert bool(sb["memory"][n0].any()) and bool((sb["memory"][n0:] == sb["memory"][n0]).all())


# ------------------------------------------------------------------------------------------------ oracle
def test_growth_against_the_oracle():
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN
    ev, n0 = _stream(), _n0()
    small = _engine(n0, _rows(ev, 0, HALF))
    small.observe_range(0, HALF, B)
    small.grow_nodes(N1)
    r = _rows(ev, HALF, NEV)
    small.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B)
    torch.cuda.synchronize()
    small.check()
    torch.manual_seed(0)
    ref = RefTGN(N1, d, hidden=D, dropout=0.0, **FORMS["1hop_last"])
    ref.load_state_dict(_sd("1hop_last"))
    lref = RefLastNeighborLoader(N1, 10)
    src, dst = torch.from_numpy(ev["src"]), torch.from_numpy(ev["dst"])
    ev_t, ev_msg = torch.from_numpy(ev["t"]), torch.from_numpy(ev["msg"])
    ref.eval()
    ref.memory.reset_state()                             # (eval mode without the flush's cell(0, 0) rows: as the engine)
    with torch.no_grad():
        for lo in range(0, NEV, B):
            sl = slice(lo, lo + B)
            ref.memory.update_state(src[sl], dst[sl], ev_t[sl], ev_msg[sl])
            lref.insert(ev["src"][sl], ev["dst"][sl], ev["t"][sl])
    m, ld = small.model, small.loader
    _close(m.memory.memory, ref.memory.memory, TOL)
    assert torch.equal(m.memory.last_update.cpu(), ref.memory.last_update)
    assert np.array_equal(ld.neighbors.cpu().numpy(), lref.neighbors)
    assert np.array_equal(ld.e_id.cpu().numpy(), lref.e_id)
    assert np.array_equal(ld.t.cpu().numpy(), lref.t.astype(np.float32))


# ------------------------------------------------------------------------------------------------ bindings
def test_bound_eval_pass_is_rebound_by_growth():
    """grow_nodes makes the resident eval binding again (its rows still exist): the pass goes on from its cursor with
    the reciprocal ranks it has, and a captured eval graph is dropped."""
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)                # (a bound split names only rows the engine has nodes for)
    lo = HALF - 4 * B
    negs = torch.from_numpy(np.random.default_rng(9).integers(0, n0, size=(HALF - lo, KN)))
    for e in (small, twin):
        e.observe_range(0, lo, B)
        e.bind_eval_resident(lo, HALF, B, negs)
        e.capture_eval(group=0)
        e.replay_eval_n(2)
    ws = small.ws.data_ptr()
    small.grow_nodes(N1)
    assert small._ev_graphs is None and small._ev is not None and small.ws.data_ptr() != ws
    with pytest.raises(RuntimeError, match="captured eval"):
        small.replay_eval_n(1)
    for e in (small, twin):
        for _ in range(3):                                                # the other two batches and a step past the end
            e.eval_resident_step()
    torch.cuda.synchronize()
    assert torch.equal(small.eval_rr(), twin.eval_rr()) and small.eval_mrr() == twin.eval_mrr()
    assert int((small.eval_rr() > 0).sum()) == HALF - lo
    _assert_twins(small, twin)
    assert _feed((small, twin), ev, HALF, NEV) == NEV - HALF              # and the stream goes on into the new nodes
    _assert_twins(small, twin)


def _train_pair():
    ev, n0 = _stream(), _n0()
    pool = np.unique(ev["dst"][:HALF])                                    # the negative pool: the caller's statement
    assert pool.max() < n0
    half = _rows(ev, 0, HALF)                            # (a bound split names only rows the engine has nodes for)
    return ev, n0, _engine(n0, half, dst_nodes=pool), _engine(N1, half, dst_nodes=pool)


def _assert_trained_twins(a, b):
    torch.cuda.synchronize()
    a.check()
    b.check()
    sa, sb = _cpu(a.stream_state()), _cpu(b.stream_state())
    exact = ("neighbors", "e_id", "ring_t", "store_nodes", "store_arena", "last_update", "src", "dst")
    assert [k for k in same_state(sa, sb) if k in exact] == []
    _close(sa["memory"], sb["memory"], 1e-4)
    _close(a.model.flat, b.model.flat, 2e-5)


def test_captured_train_graph_is_dropped_and_training_goes_on():
    ev, n0, small, twin = _train_pair()
    for e in (small, twin):
        e.bind_resident(0, HALF, B, dropout=False)
        e.begin_epoch()
        e.capture_resident()
        e.replay_resident()
        e.replay_resident()                                               # batches 0, 1; batch 2 prepared ahead
    assert small._graphs is not None and small._prefetched and small.plan_table is not None
    pt = small.plan_table.data_ptr()
    flat = small.model.flat.clone()
    small.grow_nodes(N1)
    assert small._graphs is None and not small._prefetched and hasattr(small, "_res_buf")
    assert small.plan_table is not None and small._res == (0, HALF, B)    # bound again, plan table rebuilt
    assert torch.equal(small.model.flat, flat) and pt is not None
    assert small.dst_nodes.numel() == twin.dst_nodes.numel()              # not extended
    for e in (small, twin):
        e.resident_train_step()                                           # eager, prepares its batch itself
        e.capture_resident()
        e.replay_resident()
    assert int(small.ctl[10]) == int(twin.ctl[10]) == 4
    _assert_trained_twins(small, twin)


def test_growth_and_observe_between_two_prefetched_steps():
    ev, n0, small, twin = _train_pair()
    twin.pipeline = twin.gather_ahead = False                             # the twin never prepares a batch ahead
    for e in (small, twin):
        e.bind_resident(0, HALF, B, dropout=False)
        e.begin_epoch()
        e.resident_train_step()
        e.resident_train_step()
    assert small._prefetched and not twin._prefetched
    small.grow_nodes(N1)
    assert not small._prefetched
    r = _rows(ev, 8 * B, 9 * B)                                           # rows that name grown nodes
    assert _nodes_in(ev, 8 * B, 9 * B) > n0
    for e in (small, twin):
        assert e.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B) == (HALF, B)
        assert not e._prefetched
        e.resident_train_step()
    assert small._prefetched
    _assert_trained_twins(small, twin)


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoints_across_node_counts():
    ev, n0 = _stream(), _n0()
    small, twin = _pair(ev, n0, N1, HALF)
    for e in (small, twin):
        e.observe_range(0, HALF, B)
    at_n0 = small.stream_state()
    small.grow_nodes(N1)
    assert _feed((small, twin), ev, HALF, NEV) == NEV - HALF
    want = _assert_twins(small, twin)
    grown = small.stream_state()
    one = _rows(ev, 0, 1)
    # grown -> a fresh 300-node engine, strict
    f300 = _engine(N1, one)
    f300.load_stream_state(grown)
    assert same_state(want, _cpu(f300.stream_state())) == []
    # grown -> a fresh N0 engine: only the relaxed load takes it, and grows the engine first
    f0 = _engine(n0, one)
    with pytest.raises(ValueError, match="fingerprint"):
        f0.load_stream_state(grown)
    assert int(f0.cfg.num_nodes) == n0
    f0.load_stream_state_grow(grown)
    assert int(f0.cfg.num_nodes) == N1 and same_state(want, _cpu(f0.stream_state())) == []
    # a state saved at N0 -> a 300-node engine that has a history of its own: rows >= N0 become reset rows
    with pytest.raises(ValueError, match="fingerprint"):
        f300.load_stream_state(at_n0)
    f300.load_stream_state_grow(at_n0)
    got = _cpu(f300.stream_state())
    assert same_state(pad_state(_cpu(at_n0), N1), got) == []
    assert is_reset_rows(crop_state(got, n0)[1]) and f300.num_events == HALF
    assert _feed((f300,), ev, HALF, NEV) == NEV - HALF
    _assert_twins(f300, twin)
    bad = dict(grown, ring=4)
    with pytest.raises(ValueError, match="fingerprint"):
        f0.load_stream_state_grow(bad)
    q = _query_nodes(n0, N1)                             # (last: embed advances GEN by one per call)
    want = twin.embed(q)
    assert torch.equal(f0.embed(q), want)
    assert torch.equal(f300.embed(q), want)


# ------------------------------------------------------------------------------------------------ drop-in, stand-alone
def test_dropin_observe_grow_equals_a_hand_grown_twin():
    import pyg_epoch_utils
    from tgnx import tgn_epoch
    from tgnx.data import SplitLoader, TemporalData
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TGNModel
    ev, n0 = _stream(), _n0()
    data = TemporalData(src=torch.from_numpy(ev["src"][:HALF]), dst=torch.from_numpy(ev["dst"][:HALF]),
                        t=torch.from_numpy(ev["t"][:HALF]), msg=torch.from_numpy(ev["msg"][:HALF]))
    loader = SplitLoader(data, 0, 4 * B, B, np.zeros(4 * B, dtype=np.int64))
    model = TGNModel(n0, HALF, d, D, DEV, ring=10, max_batch=B, max_neg=KN, aggr="last", dropout=0.0)
    model.load_reference_state(_sd("1hop_last"))
    nl = LastNeighborLoader(n0, 10, device=DEV)
    sampler = types.SimpleNamespace(dst_nodes=np.unique(ev["dst"][:HALF]), seed=7)
    tgn_epoch.train(model, None, loader, nl, sampler, None, DEV, TgnAdam(model, 1e-3), None)
    eng = model._tgnx_engine
    assert eng._mode_train and int(eng.cfg.num_nodes) == n0
    twin = _engine(n0, _rows(ev, 0, HALF), dst_nodes=sampler.dst_nodes)
    torch.cuda.synchronize()
    with torch.no_grad():
        for x, y in ((twin.model.memory.memory, model.memory.memory), (twin.model.memory.last_update, model.memory.last_update),
                     (twin.model.store, model.store), (twin.model.node_gen, model.node_gen), (twin.model.flat, model.flat),
                     (twin.loader.neighbors, nl.neighbors), (twin.loader.e_id, nl.e_id), (twin.loader.t, nl.t),
                     (twin.ctl, eng.ctl)):
            x.copy_(y)
    r = _rows(ev, HALF, HALF + 120)
    need = _nodes_in(ev, HALF, HALF + 120)
    assert need > n0
    with pytest.raises(ValueError, match="node ids"):
        pyg_epoch_utils.observe(model, nl, r["src"], r["dst"], r["t"], r["msg"])
    assert int(eng.cfg.num_nodes) == n0 and eng.num_events == HALF        # refused (after the switch to eval)
    twin.flush()
    assert twin.grow_nodes(need) == need
    want = twin.observe_events(r["src"], r["dst"], r["t"], r["msg"])
    got = pyg_epoch_utils.observe_grow(model, nl, r["src"], r["dst"], r["t"], r["msg"])
    assert got == want == (HALF, 120) and nl.cur_e_id == HALF + 120 and not eng._mode_train
    assert model.num_nodes == nl.num_nodes == need and model.memory.memory.shape == (need, D)
    _assert_twins(eng, twin)
    assert pyg_epoch_utils.grow_nodes(model, nl, need + 9) == need + 9 == twin.grow_nodes(need + 9)
    _assert_twins(eng, twin)
    # and the train loop goes on over its bound split with the grown node space (graphs captured again)
    tgn_epoch.train(model, None, loader, nl, sampler, None, DEV, TgnAdam(model, 1e-3), None)
    eng.check()


def test_model_and_loader_grow_on_their_own():
    """Without an engine: LastNeighborLoader.grow on the __call__ / insert path and TGNModel.grow_nodes equal objects
    built at the larger size; an engine bound afterwards runs."""
    from tgnx import tgn_epoch
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TGNModel
    ev, n0 = _stream(), _n0()
    a, b = LastNeighborLoader(n0, 10, device=DEV), LastNeighborLoader(N1, 10, device=DEV)
    for ld in (a, b):
        for lo in range(0, HALF, B):
            ld.insert(ev["src"][lo:lo + B], ev["dst"][lo:lo + B], ev["t"][lo:lo + B])
    v = a.version
    assert a.grow(n0) == n0 and a.version == v
    assert a.grow(N1) == N1 and a.num_nodes == N1 and a.version == v + 1 and a._ws_q == -1
    for ld in (a, b):
        for lo in range(HALF, NEV, B):
            ld.insert(ev["src"][lo:lo + B], ev["dst"][lo:lo + B], ev["t"][lo:lo + B])
    for k in ("neighbors", "e_id", "t"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    q = torch.from_numpy(_query_nodes(n0, N1))
    for x, y in zip(a(q), b(q)):
        assert torch.equal(x, y)
    model = TGNModel(n0, HALF, d, D, DEV, ring=10, max_batch=B, max_neg=KN, dropout=0.0)
    flat = model.flat.clone()
    with torch.no_grad():
        model.memory.memory.copy_(torch.arange(n0 * D, device=DEV).view(n0, D))
        model.store[:4 * n0].copy_(torch.arange(4 * n0, device=DEV) % 3)            # runs inside the arena
        model.store[4 * n0:].copy_(torch.arange(2 * HALF, device=DEV))
    mem, st = model.memory.memory.clone(), model.store.clone()
    c = LastNeighborLoader(n0, 10, device=DEV)
    assert tgn_epoch.grow_nodes(model, c, n0 + 31) == n0 + 31 and c.num_nodes == n0 + 31
    assert model.memory.memory.shape == (n0 + 31, D) and torch.equal(model.memory.memory[:n0], mem)
    assert not model.memory.memory[n0:].any() and not model.node_gen.any() and model.node_gen.shape == (n0 + 31,)
    assert torch.equal(model.store[:4 * n0], st[:4 * n0]) and not model.store[4 * n0:4 * (n0 + 31)].any()
    assert torch.equal(model.store[4 * (n0 + 31):], st[4 * n0:]) and torch.equal(model.flat, flat)
    assert set(model.state_dict()) >= {"memory.memory", "memory.last_update"}
    with torch.no_grad():                                                 # a run outside the arena: counted, refused
        model.store[1] = 2 * HALF + 1
    with pytest.raises(RuntimeError, match="outside the arena"):
        model.grow_nodes(n0 + 40)
    assert model.num_nodes == n0 + 31 and model.memory.memory.shape == (n0 + 31, D)
