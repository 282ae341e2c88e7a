"""Gather-ahead parity-set steps (TgnEngine.gather_ahead; include/tgnx.h TGNX_TGN_NO_GATHER_AHEAD): the next batch's
parameter-free message rows are gathered inside the step's fixup launch (GatherJob), memory / last_update are written
one launch earlier, and the next step starts with tgn_enc_fill (the time-encoding columns from its own te_w / te_b)
instead of tgn_agg_emit.  "Old path" below is the same engine class with gather_ahead = False.

With lr = 0 the parameters never move and memory comes only from the forward's GRU rows, so the float atomics of the
backward cannot reach anything compared: the two paths must then agree bit for bit (outputs, memory, last_update, ring,
stores, drawn negatives).  With the parameters moving they agree within the step's own run-to-run drift, measured
between two old-path engines (the method and floors of tests/test_gpu_tgn_group.py).

Streams are small make_stream ones with the wiki model dims (d = 172, D = 100): M and E are then no multiples of the
GEMM tiles and enc0 = 372 falls inside a 16-wide K slab."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _stream(N, nev, d, seed=3):
    from tgnx.synth import make_stream
    return make_stream("tgbl-wiki", seed=seed, num_events=nev, num_nodes=N, msg_dim=d)


def _engine(s, N, B, split, on, lr=0.0, d=172, D=100, dropout=0.1, capture=True, **model_kw):
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    kw = dict(ring=10, max_batch=B, max_neg=1, aggr="last", dropout=dropout)
    kw.update(model_kw)
    model = TGNModel(N, s.num_events, d, D, dev, **kw)
    eng = TgnEngine(model, LastNeighborLoader(N, 10, device=dev),
                    dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), TgnAdam(model, lr),
                    dst_nodes=s.dst_nodes, seed=7)
    eng.gather_ahead = on
    eng.bind_resident(0, split, B, dropout=dropout > 0)
    eng.begin_epoch()
    if capture:
        eng.capture_resident()
    return eng


def _same_state(a, b, tag):
    """Everything a step leaves behind, bit for bit."""
    torch.cuda.synchronize()
    a.check()
    b.check()
    for w in (0, 2, 3, 4, 10):                                # batch start, B, GEN, ADAM_T, NB
        assert int(a.ctl[w]) == int(b.ctl[w]), (tag, w)
    B = int(a.ctl[16])                                        # TGNX_CTL_STEP_B: the batch the step ran
    pairs = [("out_pos", a.out_pos[:B], b.out_pos[:B]), ("out_neg", a.out_neg[:B], b.out_neg[:B]),
             ("memory", a.model.memory.memory, b.model.memory.memory),
             ("last_update", a.model.memory.last_update, b.model.memory.last_update),
             ("ring.nbr", a.loader.neighbors, b.loader.neighbors), ("ring.e_id", a.loader.e_id, b.loader.e_id),
             ("ring.t", a.loader.t, b.loader.t), ("store", a.model.store, b.model.store),
             ("neg", a.neg_train, b.neg_train), ("params", a.model.flat, b.model.flat)]
    for name, x, y in pairs:
        assert torch.equal(x, y), (tag, name, float((x.double() - y.double()).abs().max()))


def test_forward_trajectory_bit_exact():
    """12 steps at lr = 0, attention dropout on: 2 eager (the first runs the non-prefetched prologue), then graph
    replay.  Pins the cosines of tgn_enc_fill against agg_node / the edge part, the zero rows of message-less nodes
    (the first batches), the memory write moved to the dW_cell launch, and the gather's read-after-write ordering."""
    N, B, nb = 300, 50, 13
    s = _stream(N, B * nb, 172)
    new, old = _engine(s, N, B, B * nb, True), _engine(s, N, B, B * nb, False)
    for st in range(12):
        for e in (new, old):
            if st < 2:
                e.resident_train_step()
            else:
                e.replay_resident()
        _same_state(new, old, st)
    assert float(new.model.memory.memory.abs().max()) > 0   # (the steps did something)


def test_parameters_moving_within_drift():
    """lr = 1e-3 on the wiki-shaped stream of tests/test_gpu_tgn_group.py: three engines (old, new, old again as the
    drift reference), 2 + 24 replayed steps.  last_update / ring / stores exact; memory, parameters, Adam moments and
    the loss within max(floor, 20 x old-vs-old drift).  A gather or an encoding that used te_w / te_b from before the
    Adam update would show here: its effect scales with lr · Δt, far above the drift."""
    from tgnx.synth import make_stream
    N, B, NB = 9_227, 200, 30
    s = make_stream("tgbl-wiki", seed=3, num_events=B * NB)
    span = max(float(s.t[-1] - s.t[0]), 1.0)
    s.t = np.floor((s.t - s.t[0]) * (2000.0 / span))
    a = _engine(s, N, B, B * NB, False, lr=1e-3)
    b = _engine(s, N, B, B * NB, True, lr=1e-3)
    c = _engine(s, N, B, B * NB, False, lr=1e-3)
    for _ in range(26):
        for e in (a, b, c):
            e.replay_resident()
    for e in (a, b, c):
        e.check()
    torch.cuda.synchronize()
    ma, mb = a.model, b.model
    assert torch.equal(ma.memory.last_update, mb.memory.last_update)
    assert torch.equal(a.loader.e_id, b.loader.e_id) and torch.equal(ma.store, mb.store)
    rel = lambda u, v: float((u.double() - v.double()).norm() / (v.double().norm() + 1e-12))

    def drift(x, y):
        return (float((x.model.memory.memory - y.model.memory.memory).abs().max()), rel(x.model.flat, y.model.flat),
                rel(x.adam_m, y.adam_m), rel(x.adam_v, y.adam_v), abs(x.loss_sum() - y.loss_sum()) / abs(y.loss_sum()))
    got, noise = drift(b, a), drift(c, a)
    print("gather-ahead vs old:", got, "old vs old:", noise)
    for name, g, n, floor in zip(("memory", "params", "adam_m", "adam_v", "loss"), got, noise,
                                 (1e-4, 2e-5, 1e-3, 1e-3, 1e-4)):
        assert g <= max(floor, 20 * n), (name, g, n)


@pytest.mark.parametrize("grouped", [False, True])
def test_boundaries_bit_exact(grouped):
    """A split whose last batch is partial (7 x 50 + 20 events), one step past it (B = 0: the gather finds no next
    batch), then begin_epoch() and a second epoch; per-step replay, and 8-step graph groups."""
    N, B, split = 300, 50, 7 * 50 + 20
    s = _stream(N, split, 172)
    new, old = _engine(s, N, B, split, True), _engine(s, N, B, split, False)
    if grouped:
        assert new.capture_group(8) and old.capture_group(8)
    for epoch in range(2):
        if grouped:
            for n in (2, 8):                 # 2 single steps (back at parity 0), then one whole 8-step group: the
                                             # 8 batches and two steps past the split
                new.replay_resident_n(n)
                old.replay_resident_n(n)
                _same_state(new, old, (epoch, n))
        else:
            for st in range(9):
                new.replay_resident()
                old.replay_resident()
                _same_state(new, old, (epoch, st))
        assert int(new.ctl[2]) == 0          # past the split
        new.begin_epoch()
        old.begin_epoch()


def test_invalidation_bit_exact():
    """Train steps interleaved with eval_batch, flush(), a loader reset and model.load_state_dict(model.state_dict()):
    the step after each prepares its batch again (mark + scan + the gather's own launch) and matches the old path.
    Then a step issued with the wrong parity still raises the stale-set error."""
    N, B, nb = 300, 50, 12
    s = _stream(N, B * nb, 172)
    new, old = _engine(s, N, B, B * nb, True, max_neg=3), _engine(s, N, B, B * nb, False, max_neg=3)
    rng = np.random.default_rng(1)
    negs = torch.from_numpy(rng.integers(0, N, size=(B, 3)))

    def between(e, st):
        if st == 2:
            e.eval_batch(st * B, B, negs)
        elif st == 4:
            e.flush()
        elif st == 6:
            e.loader.reset_state()
        elif st == 8:
            e.model.load_state_dict(e.model.state_dict())
    for st in range(10):
        for e in (new, old):
            between(e, st)
            if st in (2, 4, 6, 8):
                assert not e._prefetch_valid(), st
            e.replay_resident()
        _same_state(new, old, st)
    mem, flat = new.model.memory.memory.clone(), new.model.flat.clone()
    new._pre(True, new._parity ^ 1)          # that set holds the previous batch
    torch.cuda.synchronize()
    assert int(new.ctl[11]) & 16
    assert torch.equal(new.model.memory.memory, mem) and torch.equal(new.model.flat, flat)
    with pytest.raises(RuntimeError):
        new.check()


def test_scalar_operand_path_bit_exact():
    """msg_dim no multiple of 4 (d = 6, D = 12): vec4() is false and the element-wise operand loaders run."""
    N, B, nb = 60, 16, 9
    s = _stream(N, B * nb, 6)
    new = _engine(s, N, B, B * nb, True, d=6, D=12)
    old = _engine(s, N, B, B * nb, False, d=6, D=12)
    for st in range(8):
        for e in (new, old):
            if st < 2:
                e.resident_train_step()
            else:
                e.replay_resident()
        _same_state(new, old, st)


@pytest.mark.parametrize("form", ["mean", "two_hops", "dyrep_emb", "rnn"])
def test_other_forms_keep_the_old_path(form):
    """MeanAggregator, 2 hops, DyRep embedding messages and the RNN cell stay on tgn_agg_emit whatever the switch says:
    3 steps with it on against off, within the drift rule of test_parameters_moving_within_drift (old vs old)."""
    kw = {"mean": dict(aggr="mean"), "two_hops": dict(layers=2), "rnn": dict(updater="rnn"),
          "dyrep_emb": dict(memory="dyrep", updater="rnn", use_src_emb_in_msg=True, use_dst_emb_in_msg=True)}[form]
    N, B, nb = 300, 50, 5
    s = _stream(N, B * nb, 172)
    a, b, c = (_engine(s, N, B, B * nb, on, lr=1e-3, **kw) for on in (False, True, False))
    for _ in range(3):
        for e in (a, b, c):
            e.replay_resident()
    for e in (a, b, c):
        e.check()
    torch.cuda.synchronize()
    assert torch.equal(a.model.memory.last_update, b.model.memory.last_update)
    assert torch.equal(a.loader.e_id, b.loader.e_id) and torch.equal(a.model.store, b.model.store)
    rel = lambda u, v: float((u.double() - v.double()).norm() / (v.double().norm() + 1e-12))

    def drift(x, y):
        return (float((x.model.memory.memory - y.model.memory.memory).abs().max()), rel(x.model.flat, y.model.flat),
                rel(x.adam_m, y.adam_m), rel(x.adam_v, y.adam_v), abs(x.loss_sum() - y.loss_sum()) / abs(y.loss_sum()))
    got, noise = drift(b, a), drift(c, a)
    for name, g, n, floor in zip(("memory", "params", "adam_m", "adam_v", "loss"), got, noise,
                                 (1e-4, 2e-5, 1e-3, 1e-3, 1e-4)):
        assert g <= max(floor, 20 * n), (form, name, g, n)
