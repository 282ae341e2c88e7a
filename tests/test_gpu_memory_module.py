"""GPU parity of tgnx.nn.TGNMemory / DyRepMemory (device message store, csrc/tgnx_memstore.hip) against the CPU
restatement oracle/tgn_ref.RefTGNMemory and the reference goldens tests/golden/tgn_memory_*.npz.

Tolerances are tests/test_gpu_nn_modules.py's: FWD_TOL 2e-5 on values, GRAD_TOL 1e-4 on gradients, errors scaled by
max(|ref|, 1); integers (last_update, store counts, store order, owner order) are exact."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
LR, ADAM_EPS = 1e-3, 1e-8


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if not b.numel():
        return 0.0
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1.0)


def _close(a, b, tol, what=""):
    e = _err(a, b)
    print(f"{what}: scaled err {e:.3e} tol {tol:g}")
    assert e <= tol, (what, e, tol)


def _exact(a, b, what=""):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


def _adam_close(p_gpu, p_ref, g_ref, what):
    """tests/test_gpu_nn_modules.py::_adam_close: the first Adam step moves p by lr u(g), u(g) = g / (|g| + eps)."""
    p_gpu, p_ref, g = p_gpu.detach().double().cpu(), p_ref.detach().double(), g_ref.detach().double()
    delta = GRAD_TOL * max(float(g.abs().max()), 1.0)
    u = lambda x: x / (x.abs() + ADAM_EPS)  # noqa: E731
    bound = LR * torch.maximum((u(g + delta) - u(g)).abs(), (u(g - delta) - u(g)).abs())
    bound = bound + 1e-6 * p_ref.abs().clamp(min=1.0)
    excess = float(((p_gpu - p_ref).abs() - bound).max())
    print(f"{what}: max |dp| {float((p_gpu - p_ref).abs().max()):.3e}, over bound by {excess:.3e}")
    assert excess <= 0.0, (what, excess)


def _gpu_memory(N, d, D, T, aggr, cell, msg=None, cls=None, **kw):
    from tgnx import nn as tnn
    cls = cls or tnn.TGNMemory
    agg = tnn.LastAggregator() if aggr == "last" else tnn.MeanAggregator()
    return cls(N, d, D, T, msg if msg is not None else tnn.IdentityMessage(d, D, T), agg, cell, **kw)


def _store_state(mem):
    cs, _, _, ts, _ = mem.message_store("s")
    cd, _, _, _, _ = mem.message_store("d")
    return cs.cpu().numpy(), cd.cpu().numpy(), ts.cpu().numpy()


# ------------------------------------------------------------------ 1. reference goldens
@pytest.mark.parametrize("aggr,updater", [("last", "gru"), ("mean", "gru"), ("last", "rnn")])
def test_reference_goldens(golden, aggr, updater):
    """tests/test_oracle_goldens.py::test_tgn_memory_oracle_matches_reference_module replayed with the HIP module in
    place of the oracle (N = 40, d = 5, D = T = 8, B = 12: message width 29, every column group unaligned — the
    element-wise path of the build kernel): 5 train batches, the train(False) flush, 2 eval batches; after every call
    z and both buffers at FWD_TOL + 2e-6 (what the oracle itself is allowed against the golden), lu, last_update and
    the stores' sizes and the s stores' times (message_store) exactly."""
    z = golden(f"tgn_memory_{aggr}_{updater}.npz")
    N, d, D, B, n_train, n_eval = z["meta"].tolist()
    tol = FWD_TOL + 2e-6
    mem = _gpu_memory(N, d, D, D, aggr, updater)
    sd = {k[2:].replace("__", "."): torch.from_numpy(z[k]) for k in z.files if k.startswith("p_")}
    res = mem.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"memory", "last_update", "_assoc"}
    mem = mem.to(DEV).train()
    for b in range(n_train + n_eval):
        if b == n_train:
            mem.train(False)
            _close(mem.memory, torch.from_numpy(z["flush_memory"]), tol, "flush memory")
            _exact(mem.last_update, torch.from_numpy(z["flush_last_update"]), "flush last_update")
            cs, cd, ts = _store_state(mem)
            assert not cs.any() and not cd.any() and ts.size == 0
        s, dd = torch.from_numpy(z["src"][b]), torch.from_numpy(z["dst"][b])
        n_id = torch.cat([s, dd, torch.from_numpy(z["extra"][b])]).unique()
        np.testing.assert_array_equal(n_id.numpy(), z[f"b{b}_nid"])
        with torch.no_grad():
            zz, lu = mem(n_id.to(DEV))
            _close(zz, torch.from_numpy(z[f"b{b}_z"]), tol, f"batch {b} z")
            _exact(lu, torch.from_numpy(z[f"b{b}_lu"]), f"batch {b} lu")
            mem.update_state(s.to(DEV), dd.to(DEV), torch.from_numpy(z["t"][b]).to(DEV),
                             torch.from_numpy(z["msg"][b]).to(DEV))
        _close(mem.memory, torch.from_numpy(z[f"b{b}_memory"]), tol, f"batch {b} memory")
        _exact(mem.last_update, torch.from_numpy(z[f"b{b}_last_update"]), f"batch {b} last_update")
        cs, cd, ts = _store_state(mem)
        np.testing.assert_array_equal(cs, z[f"b{b}_store_s_n"])
        np.testing.assert_array_equal(cd, z[f"b{b}_store_d_n"])
        np.testing.assert_array_equal(ts.astype(np.float64), z[f"b{b}_store_s_t"])


def test_flush_in_chunks_matches_golden(golden):
    """train(False) on a graph larger than one flush chunk walks the nodes in chunks (here 16 of the 40), every row
    computed from the pre-flush state: the golden's flush result."""
    z = golden("tgn_memory_last_gru.npz")
    N, d, D, B, n_train, n_eval = z["meta"].tolist()
    mem = _gpu_memory(N, d, D, D, "last", "gru")
    mem.load_state_dict({k[2:].replace("__", "."): torch.from_numpy(z[k]) for k in z.files if k.startswith("p_")},
                        strict=False)
    mem = mem.to(DEV).train()
    mem._FLUSH_CHUNK = 16
    with torch.no_grad():
        for b in range(n_train):
            mem.update_state(*(torch.from_numpy(z[k][b]).to(DEV) for k in ("src", "dst", "t", "msg")))
    mem.train(False)
    _close(mem.memory, torch.from_numpy(z["flush_memory"]), FWD_TOL + 2e-6, "chunked flush memory")
    _exact(mem.last_update, torch.from_numpy(z["flush_last_update"]), "chunked flush last_update")
    assert mem._fill == 0 and not bool(mem._node_tab.any())


# ------------------------------------------------------------------ 2. oracle parity at wiki's dimensions
WN, Wd, WD, WB, W_TRAIN = 1000, 172, 100, 300, 4
HUB = 7


def _wiki_batches():
    """W_TRAIN train batches + one for after reset_state.  Node HUB is src of 150 and dst of 100 events of batch 1
    (more than a wavefront of stored events under one owner) and appears again in batch 2 (its runs are replaced);
    batch 0 has two self-loops; ids >= 900 are never seen but queried; times repeat (ties for LastAggregator)."""
    rng = np.random.default_rng(7)
    out, t0 = [], 0
    for b in range(W_TRAIN + 1):
        src, dst = rng.integers(0, 900, WB), rng.integers(0, 900, WB)
        src[src == HUB], dst[dst == HUB] = 8, 8
        if b == 0:
            dst[3], dst[200] = src[3], src[200]
        if b == 1:
            idx = rng.permutation(WB)
            src[idx[:150]], dst[idx[150:250]] = HUB, HUB
        if b == 2:
            src[5], dst[17] = HUB, HUB
        t = t0 + np.sort(rng.integers(0, 2000, WB)) * 300
        t0 = int(t.max())
        msg = rng.standard_normal((WB, Wd)).astype(np.float32)
        extra = np.concatenate([rng.integers(0, WN, 40), [950, 999, HUB]])
        n_id = np.unique(np.concatenate([src, dst, extra]))
        out.append(tuple(torch.from_numpy(x) for x in (src, dst, t.astype(np.int64), msg, n_id)))
    assert int((out[1][0] == HUB).sum()) == 150 and int((out[1][1] == HUB).sum()) == 100
    assert int((out[0][0] == out[0][1]).sum()) >= 2 and bool((out[0][4] >= 900).any())
    return out


def _run_wiki(mem, batches, dev, edge_calls=False):
    """The sequence of test 2 on either side: per train batch forward(n_id) and update_state (with one empty n_id and
    one empty batch in between with edge_calls: neither changes any state), then the flush.  Returns every observed
    tensor, in order."""
    seen = []
    mem.train()
    with torch.no_grad():
        for b in range(W_TRAIN):
            src, dst, t, msg, n_id = (x.to(dev) for x in batches[b])
            z, lu = mem(n_id)
            seen += [(f"b{b} z", z), (f"b{b} lu", lu)]
            if b == 1 and edge_calls:
                z0, lu0 = mem(n_id[:0])
                assert z0.shape == (0, WD) and lu0.shape == (0,) and lu0.dtype == torch.long
                mem.update_state(src[:0], dst[:0], t[:0], msg[:0])
            mem.update_state(src, dst, t, msg)
            seen += [(f"b{b} memory", mem.memory.clone()), (f"b{b} last_update", mem.last_update.clone())]
        mem.train(False)
        seen += [("flush memory", mem.memory.clone()), ("flush last_update", mem.last_update.clone())]
    return seen


_WIKI = {}


def _wiki_reference():
    """(batches, state dict, the float32 oracle's observations, d64), computed once."""
    if _WIKI:
        return _WIKI["v"]
    from oracle.tgn_ref import RefTGNMemory
    batches = _wiki_batches()
    torch.manual_seed(3)
    ref = RefTGNMemory(WN, Wd, WD, WD, aggr="last", updater="gru")
    sd = copy.deepcopy(ref.state_dict())
    seen32 = _run_wiki(ref, batches, "cpu")
    torch.set_default_dtype(torch.float64)
    try:
        ref64 = RefTGNMemory(WN, Wd, WD, WD, aggr="last", updater="gru")
        ref64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        b64 = [(s, d_, t, m.double(), n) for s, d_, t, m, n in batches]
        seen64 = _run_wiki(ref64, b64, "cpu")
    finally:
        torch.set_default_dtype(torch.float32)
    d64 = max(_err(a, b) for (_, a), (_, b) in zip(seen32, seen64) if a.is_floating_point())
    _WIKI["v"] = (batches, sd, seen32, d64)
    return _WIKI["v"]


def _run_wiki_gpu(store_capacity=64):
    batches, sd, _, _ = _wiki_reference()
    mem = _gpu_memory(WN, Wd, WD, WD, "last", "gru", store_capacity=store_capacity)
    mem.load_state_dict(sd, strict=True)
    mem = mem.to(DEV)
    return mem, _run_wiki(mem, batches, DEV, edge_calls=True)


def test_oracle_parity_wiki_dimensions():
    """N = 1,000, d = 172, D = T = 100 (width 472: every column group moves as 16-B vectors), four train batches of
    300 from a store capacity of 64 (the first batch grows it), nothing resynchronised: every returned row, both
    buffers after every call, the flush; then reset_state() and one more batch, bit for bit a fresh module's.
    Bound: FWD_TOL for the first batch, max(FWD_TOL, 4 d64) afterwards, d64 = the float32 oracle against the float64
    oracle over the same sequence on CPU (measured: 8.8e-07, so 4 d64 = 3.5e-06 and the bound is FWD_TOL)."""
    batches, sd, seen32, d64 = _wiki_reference()
    print(f"d64 = {d64:.3e}")
    bound = max(FWD_TOL, 4 * d64)
    mem, seen = _run_wiki_gpu()
    assert mem._log_src.numel() >= W_TRAIN * WB and mem._fill == 0
    assert len(seen) == len(seen32)
    for (what, got), (_, want) in zip(seen, seen32):
        if want.is_floating_point():
            _close(got, want, FWD_TOL if what.startswith("b0 ") else bound, what)
        else:
            _exact(got, want, what)
    # reset_state, one more batch: equal to a fresh module's, bit for bit
    src, dst, t, msg, n_id = (x.to(DEV) for x in batches[W_TRAIN])
    mem.reset_state()
    mem.train()
    fresh = _gpu_memory(WN, Wd, WD, WD, "last", "gru")
    fresh.load_state_dict({k: v for k, v in sd.items() if k not in ("memory", "last_update", "_assoc")}, strict=False)
    fresh = fresh.to(DEV).train()
    outs = []
    for m in (mem, fresh):
        with torch.no_grad():
            m.update_state(src, dst, t, msg)
            z, lu = m(n_id)
            m.update_state(src, dst, t + 5, msg)
        outs.append((z, lu, m.memory.clone(), m.last_update.clone(), *m.message_store("d")))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][2].abs().max()) > 0


# ------------------------------------------------------------------ 3. gradients
GN, Gd, GD, GT, GB = 80, 6, 12, 10, 30     # width 40: memory columns as vectors, raw and time columns element-wise


class _LinearMessage(torch.nn.Module):
    """A user message module with a parameter: Linear over the concatenation of the four inputs."""

    def __init__(self, in_dim, out_channels):
        super().__init__()
        self.out_channels = out_channels
        self.lin = torch.nn.Linear(in_dim, out_channels)

    def forward(self, z_src, z_dst, raw_msg, t_enc):
        return self.lin(torch.cat([z_src, z_dst, raw_msg, t_enc], dim=-1))


def _ref_with_message(N, d, D, T, msg_module, aggr, updater):
    """RefTGNMemory with `msg_module` applied to the pieces its _compute_msg concatenates."""
    from oracle import tgn_ref as R

    class RefWithMessage(R.RefTGNMemory):
        def _get_updated_memory(self, n_id, embeddings=None, assoc=None):
            self._assoc[n_id] = torch.arange(n_id.size(0))
            cat_s, t_s, src_s, _ = self._compute_msg(n_id, self.msg_s_store)
            cat_d, t_d, src_d, _ = self._compute_msg(n_id, self.msg_d_store)
            cols = lambda c: (c[:, :D], c[:, D:2 * D], c[:, 2 * D:2 * D + d], c[:, 2 * D + d:])  # noqa: E731
            msg = torch.cat([self.msg_s_module(*cols(cat_s)), self.msg_d_module(*cols(cat_d))], dim=0)
            idx, t = torch.cat([src_s, src_d]), torch.cat([t_s, t_d])
            agg = R.last_aggregate if self.aggr == "last" else R.mean_aggregate
            memory = self.memory_updater(agg(msg, self._assoc[idx], t, n_id.size(0)), self.memory[n_id])
            last_update, _ = R.scatter_max_first(t, idx, self.num_nodes)
            return memory, last_update[n_id]

    ref = RefWithMessage(N, d, D, T, aggr=aggr, updater=updater)
    ref.msg_s_module, ref.msg_d_module = msg_module, copy.deepcopy(msg_module)
    ref.memory_updater = (torch.nn.GRUCell if updater == "gru" else torch.nn.RNNCell)(msg_module.out_channels, D)
    return ref


def _grad_batches(seed):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(2):
        src, dst = rng.integers(0, GN - 10, GB), rng.integers(0, GN - 10, GB)
        t = 1000 * b + np.sort(rng.integers(0, 40, GB)) * 25_000
        out.append((torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(t.astype(np.int64)),
                    torch.from_numpy(rng.standard_normal((GB, Gd)).astype(np.float32))))
    n_id = torch.from_numpy(np.unique(np.concatenate([out[0][0], out[1][1], rng.integers(0, GN, 20)])))
    return out, n_id


@pytest.mark.parametrize("user_msg", [False, True])
@pytest.mark.parametrize("aggr,cell", [("last", "gru"), ("mean", "gru"), ("last", "rnn"), ("mean", "rnn")])
def test_gradients_match_oracle(aggr, cell, user_msg):
    """One training forward(n_id) after two stored batches, out.backward(dout) on both sides: every parameter
    gradient (time_enc.lin.*, memory_updater.*; with the user message module also msg_s_module.* / msg_d_module.*,
    through the four column views) at GRAD_TOL."""
    from oracle.tgn_ref import RefTGNMemory
    torch.manual_seed(20)
    batches, n_id = _grad_batches(21)
    if user_msg:
        msg = _LinearMessage(2 * GD + Gd + GT, 16)
        ref = _ref_with_message(GN, Gd, GD, GT, msg, aggr, cell)
        mine = _gpu_memory(GN, Gd, GD, GT, aggr, cell, msg=copy.deepcopy(msg))
        with torch.no_grad():   # the two directions' modules differ
            ref.msg_d_module.lin.weight.mul_(0.5)
    else:
        ref = RefTGNMemory(GN, Gd, GD, GT, aggr=aggr, updater=cell)
        mine = _gpu_memory(GN, Gd, GD, GT, aggr, cell)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV)
    ref.train(), mine.train()
    for src, dst, t, raw in batches:
        ref.update_state(src, dst, t, raw)
        mine.update_state(src.to(DEV), dst.to(DEV), t.to(DEV), raw.to(DEV))
    dout = torch.randn(n_id.numel(), GD)
    want, lu_ref = ref(n_id)
    want.backward(dout)
    got, lu = mine(n_id.to(DEV))
    got.backward(dout.to(DEV))
    _close(got, want, FWD_TOL, "z")
    _exact(lu, lu_ref, "lu")
    refs = dict(ref.named_parameters())
    names = [n for n, _ in mine.named_parameters()]
    assert set(names) == set(refs)
    assert {"time_enc.lin.weight", "time_enc.lin.bias", "memory_updater.weight_ih"} <= set(names)
    assert not user_msg or {"msg_s_module.lin.weight", "msg_d_module.lin.bias"} <= set(names)
    for name, p in mine.named_parameters():
        assert p.grad is not None and refs[name].grad is not None, name
        assert float(refs[name].grad.abs().max()) > 0, name
        _close(p.grad, refs[name].grad, GRAD_TOL, f"d{name}")


# ------------------------------------------------------------------ 4. composed model
class _Model(torch.nn.Module):
    """pyg_model_utils.getModel from tgnx.nn: TGNMemory + GraphAttentionEmbedding sharing memory.time_enc + predictor."""

    def __init__(self, N, d, D):
        super().__init__()
        from tgnx import nn as tnn
        self.memory = tnn.TGNMemory(N, d, D, D, tnn.IdentityMessage(d, D, D), tnn.LastAggregator())
        self.gnn = tnn.GraphAttentionEmbedding(D, D, d, self.memory.time_enc, dropout=0.0)
        self.link_pred = tnn.LinkPredictor(D)


def test_composed_model_trains_like_oracle():
    """The reference's getModel composed from tgnx.nn, driven by the drop-in LastNeighborLoader through the loop of
    oracle.tgn_ref.train_step for 4 batches (N = 300, B = 50, d = 16, hidden = 32) against RefTGN + train_step with
    dropout 0.0.  Before every batch the parameters are reloaded from the oracle and both sides take a fresh Adam, so
    that every step is a first step, which is what _adam_close bounds; memory, last_update, the stores and the ring are
    never resynchronised.  Per batch: loss, outputs, every gradient (the shared time encoder's summed over both uses),
    the parameters after the step, memory and last_update."""
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN, train_step
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import make_stream
    N, B, d, D, NB = 300, 50, 16, 32, 4
    s = make_stream("tgbl-wiki", seed=3, num_events=B * NB, num_nodes=N, msg_dim=d)
    assert np.array_equal(s.t, np.floor(s.t)) and float(s.t.max()) < 2 ** 24     # integer times, exact in float32
    torch.manual_seed(0)
    ref = RefTGN(N, d, hidden=D, aggr="last", dropout=0.0)
    mine = _Model(N, d, D)
    assert mine.gnn.time_enc is mine.memory.time_enc
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV).train()
    lref, lgpu = RefLastNeighborLoader(N, 10), LastNeighborLoader(N, 10, device=DEV)
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    ev_t_g, ev_msg_g = ev_t.to(DEV), ev_msg.to(DEV)
    assoc = torch.zeros(N, dtype=torch.long, device=DEV)
    rng = np.random.default_rng(1)
    crit = torch.nn.BCEWithLogitsLoss()
    refs = dict(ref.named_parameters())
    for b in range(NB):
        sl = slice(b * B, (b + 1) * B)
        src, pos = torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl])
        neg = torch.from_numpy(rng.choice(s.dst_nodes, size=B))
        with torch.no_grad():
            for n, p in mine.named_parameters():
                p.copy_(refs[n].detach().to(DEV))
        opt_r = torch.optim.Adam(ref.parameters(), lr=LR, eps=ADAM_EPS)
        opt_m = torch.optim.Adam(mine.parameters(), lr=LR, eps=ADAM_EPS)
        loss_r, po, no = train_step(ref, opt_r, lref, ev_t, ev_msg, src, pos, neg, ev_t[sl], ev_msg[sl])
        # the same loop on the device
        sg, pg, ng = src.to(DEV), pos.to(DEV), neg.to(DEV)
        opt_m.zero_grad()
        n_id, ei, e_id, _ = lgpu(torch.cat([sg, pg, ng]).unique())
        assoc[n_id] = torch.arange(n_id.numel(), device=DEV)
        z, last_update = mine.memory(n_id)
        z = mine.gnn(z, last_update, ei, ev_t_g[e_id], ev_msg_g[e_id])
        pos_out = mine.link_pred(z[assoc[sg]], z[assoc[pg]])
        neg_out = mine.link_pred(z[assoc[sg]], z[assoc[ng]])
        loss = crit(pos_out, torch.ones_like(pos_out)) + crit(neg_out, torch.zeros_like(neg_out))
        mine.memory.update_state(sg, pg, ev_t_g[sl].long(), ev_msg_g[sl])
        lgpu.insert(sg, pg, ev_t_g[sl])
        loss.backward()
        _close(loss, torch.tensor(loss_r), FWD_TOL, f"batch {b} loss")
        _close(pos_out.view(-1), po, FWD_TOL, f"batch {b} pos")
        _close(neg_out.view(-1), no, FWD_TOL, f"batch {b} neg")
        grads = {}
        for n, p in mine.named_parameters():
            assert p.grad is not None, n
            _close(p.grad, refs[n].grad, GRAD_TOL, f"batch {b} d{n}")
            grads[n] = refs[n].grad.clone()
        opt_m.step()
        mine.memory.detach()
        for n, p in mine.named_parameters():
            _adam_close(p, refs[n], grads[n], f"batch {b} {n} after Adam")
        _close(mine.memory.memory, ref.memory.memory, FWD_TOL, f"batch {b} memory")
        _exact(mine.memory.last_update, ref.memory.last_update, f"batch {b} last_update")


# ------------------------------------------------------------------ 5. DyRep
@pytest.mark.parametrize("flag", ["use_src_emb_in_msg", "use_dst_emb_in_msg"])
def test_dyrep_embeddings_in_messages(flag):
    """DyRepMemory(..., 'rnn', use_src_emb_in_msg / use_dst_emb_in_msg) against RefTGNMemory with the same flag over 3
    batches, embeddings and assoc passed to update_state.  Oracle parity only: the reference goldens do not cover these
    flags.  Every batch first queries a larger node set, so _assoc holds stale stamps of nodes outside the batch's own
    node set when update_state tests membership; stored events' other endpoints are partly inside and partly outside
    that set."""
    from oracle.tgn_ref import RefTGNMemory
    from tgnx import nn as tnn
    N, d, D, T, B = 120, 6, 12, 10, 25
    torch.manual_seed(30)
    rng = np.random.default_rng(31)
    ref = RefTGNMemory(N, d, D, T, aggr="last", updater="rnn", **{flag: True})
    mine = _gpu_memory(N, d, D, T, "last", "rnn", cls=tnn.DyRepMemory, **{flag: True})
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV)
    ref.train(), mine.train()
    inside = outside = 0
    for b in range(3):
        src, dst = torch.from_numpy(rng.integers(0, 60, B)), torch.from_numpy(rng.integers(0, 60, B))
        t = torch.from_numpy((b * 2_000_000 + np.sort(rng.integers(0, 50, B)) * 30_000).astype(np.int64))
        raw = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32))
        big = torch.cat([src, dst, torch.from_numpy(rng.integers(0, N, 60))]).unique()
        small = torch.cat([src, dst]).unique()
        emb = torch.randn(big.numel(), D)
        assoc = torch.zeros(N, dtype=torch.long)
        assoc[big] = torch.arange(big.numel())
        for store in (ref.msg_s_store, ref.msg_d_store):
            for j in small.tolist():
                if j in store:
                    m = torch.isin(store[j][1], small)
                    inside, outside = inside + int(m.sum()), outside + int((~m).sum())
        with torch.no_grad():
            want, lu_r = ref(big)
            got, lu = mine(big.to(DEV))
            _close(got, want, FWD_TOL, f"{flag} batch {b} z")
            _exact(lu, lu_r, f"{flag} batch {b} lu")
            ref.update_state(src, dst, t, raw, emb, assoc)
            mine.update_state(src.to(DEV), dst.to(DEV), t.to(DEV), raw.to(DEV), emb.to(DEV), assoc.to(DEV))
        _close(mine.memory, ref.memory, FWD_TOL, f"{flag} batch {b} memory")
        _exact(mine.last_update, ref.last_update, f"{flag} batch {b} last_update")
    assert inside > 0 and outside > 0
    ref.train(False), mine.train(False)
    _close(mine.memory, ref.memory, FWD_TOL, f"{flag} flush memory")
    _exact(mine.last_update, ref.last_update, f"{flag} flush last_update")


# ------------------------------------------------------------------ 6. determinism and host traffic
def test_two_runs_are_bit_identical():
    """Test 2's sequence twice: memory, last_update and every returned row bit-identical; so are the gradients of a
    training forward after the stored batches."""
    batches, sd, _, _ = _wiki_reference()
    runs = []
    for _ in range(2):
        mem, seen = _run_wiki_gpu()
        mem.train()
        src, dst, t, msg, n_id = (x.to(DEV) for x in batches[W_TRAIN])
        with torch.no_grad():
            mem.update_state(src, dst, t, msg)
        out, _ = mem(n_id)
        out.backward(torch.ones_like(out) * torch.linspace(-1, 1, WD, device=DEV))
        runs.append([x for _, x in seen] + [out.detach()] + [p.grad for p in mem.parameters()])
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert all(float(g.abs().max()) > 0 for g in runs[0][-6:])


def test_store_update_issues_no_device_to_host_copy():
    """update_state's store update (a stable sort, one launch, a growth of the log included) under
    torch.cuda.set_sync_debug_mode('error'), which raises on any synchronising call."""
    batches, sd, _, _ = _wiki_reference()
    mem = _gpu_memory(WN, Wd, WD, WD, "last", "gru", store_capacity=64).to(DEV).train()
    src, dst, t, msg, _ = (x.to(DEV) for x in batches[0])
    mem._update_msg_store(src[:8], dst[:8], t[:8], msg[:8])     # loads the op library outside the checked region
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                        # the mode is honoured: a device -> host read raises
        mem._update_msg_store(src, dst, t, msg)                 # grows 64 -> 512, then the put
        mem._update_msg_store(dst, src, t + 1, msg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert mem._fill == 8 + 2 * WB and mem._log_src.numel() >= mem._fill
    cs, cd, ts = _store_state(mem)
    assert WB <= int(cs.sum()) <= mem._fill and WB <= int(cd.sum()) <= mem._fill and ts.size == int(cs.sum())
