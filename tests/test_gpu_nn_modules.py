"""GPU parity of the trainable modules (tgnx/nn.py) against the same composition of the oracle's restatements
(oracle/tgn_ref.py) on CPU, from the same state dict:

  TransformerConv / GraphAttentionEmbedding   eval(): output 2e-5 and every parameter's gradient 1e-4, on 60 nodes and
                                              300 unsorted edges (a node without incoming edges, one with 150)
  TransformerConv dropout                     train() with dropout 0.1 raises NotImplementedError; dropout 0.0 trains
  one composed TGN step                       TimeEncoder -> IdentityMessage -> Last / MeanAggregator -> MemoryCell
                                              (gru / rnn) -> GraphAttentionEmbedding -> LinkPredictor -> BCE -> Adam:
                                              loss, every gradient, every parameter after the step; the shared
                                              time_enc gets the sum of the message path's and the embedding's gradient
  one composed JODIE step                     MemoryCell('rnn') -> TimeEmbedding -> LinkPredictor

Errors as in module_ref.close (max |a - b| over max(|b|, 1)).  Parameters after the Adam step: the first
Adam step moves p by lr u(g), u(g) = g / (|g| + eps), which is ill-conditioned where g ~ 0, so the bound on
|p_gpu - p_ref| is lr times the change of u over the gradient tolerance, [g - δ, g + δ] with δ = 1e-4 max(|g|_max, 1)
(u is monotonic: the extremes are at the ends), plus fp32 rounding of p."""
import numpy as np
import pytest
import torch

from module_ref import close as _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
LR, ADAM_EPS = 1e-3, 1e-8


def _adam_close(p_gpu, p_ref, g_ref, what):
    p_gpu, p_ref, g = p_gpu.detach().double().cpu(), p_ref.detach().double(), g_ref.detach().double()
    delta = GRAD_TOL * max(float(g.abs().max()), 1.0)
    u = lambda x: x / (x.abs() + ADAM_EPS)  # noqa: E731
    bound = LR * torch.maximum((u(g + delta) - u(g)).abs(), (u(g - delta) - u(g)).abs())
    bound = bound + 1e-6 * p_ref.abs().clamp(min=1.0)
    excess = float(((p_gpu - p_ref).abs() - bound).max())
    print(f"{what}: max |dp| {float((p_gpu - p_ref).abs().max()):.3e}, over bound by {excess:.3e}")
    assert excess <= 0.0, (what, excess)


def _grads_close(mine: torch.nn.Module, ref: torch.nn.Module, what):
    refs = dict(ref.named_parameters())
    n = 0
    for name, p in mine.named_parameters():
        assert p.grad is not None, name
        _close(p.grad, refs[name].grad, GRAD_TOL, f"{what} d{name}")
        n += 1
    assert n == len(refs)


def _graph(seed, n_nodes=60, n_edges=300, hub=7, hub_deg=150, empty=11):
    """Unsorted edges; node `empty` has no incoming edge and node `hub` has hub_deg."""
    rng = np.random.default_rng(seed)
    others = np.array([i for i in range(n_nodes) if i not in (hub, empty)])
    dst = np.concatenate([np.full(hub_deg, hub), rng.choice(others, n_edges - hub_deg)])
    src = rng.integers(0, n_nodes, n_edges)
    perm = rng.permutation(n_edges)
    ei = torch.from_numpy(np.stack([src[perm], dst[perm]]))
    assert int((ei[1] == hub).sum()) == hub_deg and int((ei[1] == empty).sum()) == 0
    return ei


def test_transformer_conv_eval_matches_oracle():
    from oracle.tgn_ref import RefTransformerConv
    from tgnx.nn import TransformerConv
    torch.manual_seed(0)
    ref = RefTransformerConv(100, 50, 2, 0.1, 272).eval()
    mine = TransformerConv(100, 50, heads=2, dropout=0.1, edge_dim=272)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV).eval()
    ei = _graph(1)
    x, ea = torch.randn(60, 100, requires_grad=True), torch.randn(300, 272, requires_grad=True)
    dout = torch.randn(60, 100)
    want = ref(x, ei, ea)
    want.backward(dout)
    xd, ead = x.detach().to(DEV).requires_grad_(True), ea.detach().to(DEV).requires_grad_(True)
    out = mine(xd, ei.to(DEV), ead)
    out.backward(dout.to(DEV))
    _close(out, want, FWD_TOL, "conv out")
    _close(out[11], ref.lin_skip(x)[11], FWD_TOL, "conv out, node without edges = skip term")
    _close(xd.grad, x.grad, GRAD_TOL, "conv dx")
    _close(ead.grad, ea.grad, GRAD_TOL, "conv dedge_attr")
    _grads_close(mine, ref, "conv")


def test_graph_attention_embedding_eval_matches_oracle():
    from oracle.tgn_ref import RefGraphAttentionEmbedding, RefTimeEncoder
    from tgnx.nn import GraphAttentionEmbedding, TimeEncoder
    torch.manual_seed(2)
    ref = RefGraphAttentionEmbedding(100, 100, 172, RefTimeEncoder(100)).eval()
    mine = GraphAttentionEmbedding(100, 100, 172, TimeEncoder(100))
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV).eval()
    ei = _graph(3)
    rng = np.random.default_rng(4)
    x = torch.randn(60, 100, requires_grad=True)
    last_update = torch.from_numpy(rng.integers(0, 2_600_000, 60))
    t = torch.from_numpy(rng.integers(0, 2_600_000, 300))
    msg = torch.randn(300, 172)
    dout = torch.randn(60, 100)
    want = ref(x, last_update, ei, t, msg)
    want.backward(dout)
    xd = x.detach().to(DEV).requires_grad_(True)
    out = mine(xd, last_update.to(DEV), ei.to(DEV), t.to(DEV), msg.to(DEV))
    out.backward(dout.to(DEV))
    _close(out, want, FWD_TOL, "gnn out")
    _close(xd.grad, x.grad, GRAD_TOL, "gnn dx")
    _grads_close(mine, ref, "gnn")


@pytest.mark.parametrize("c_in,c_out,heads,edge_dim", [(24, 13, 3, 20), (7, 32, 8, 5)])
def test_transformer_conv_other_widths_match_oracle(c_in, c_out, heads, edge_dim):
    """heads 3 x 13 = 39 and 8 x 32 = 256 channels (one and four registers per lane in the attention kernels), on 37
    nodes (not a multiple of the four destinations a block takes) with the same hub and node without edges."""
    from oracle.tgn_ref import RefTransformerConv
    from tgnx.nn import TransformerConv
    torch.manual_seed(c_in)
    ref = RefTransformerConv(c_in, c_out, heads, 0.1, edge_dim).eval()
    mine = TransformerConv(c_in, c_out, heads=heads, dropout=0.1, edge_dim=edge_dim)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV).eval()
    ei = _graph(c_in + 1, n_nodes=37)
    x, ea = torch.randn(37, c_in, requires_grad=True), torch.randn(300, edge_dim, requires_grad=True)
    dout = torch.randn(37, heads * c_out)
    want = ref(x, ei, ea)
    want.backward(dout)
    xd, ead = x.detach().to(DEV).requires_grad_(True), ea.detach().to(DEV).requires_grad_(True)
    out = mine(xd, ei.to(DEV), ead)
    out.backward(dout.to(DEV))
    what = f"conv {c_in}->{heads}x{c_out}"
    _close(out, want, FWD_TOL, f"{what} out")
    _close(out[11], ref.lin_skip(x)[11], FWD_TOL, f"{what} out, node without edges = skip term")
    _close(xd.grad, x.grad, GRAD_TOL, f"{what} dx")
    _close(ead.grad, ea.grad, GRAD_TOL, f"{what} dedge_attr")
    _grads_close(mine, ref, what)


def test_graph_attention_embedding_other_widths_match_oracle():
    """Memory 24, time 12, raw message 5: 2 heads x 12 channels, edge_dim 17, on 37 nodes."""
    from oracle.tgn_ref import RefGraphAttentionEmbedding, RefTimeEncoder
    from tgnx.nn import GraphAttentionEmbedding, TimeEncoder
    torch.manual_seed(30)
    ref = RefGraphAttentionEmbedding(24, 24, 5, RefTimeEncoder(12)).eval()
    mine = GraphAttentionEmbedding(24, 24, 5, TimeEncoder(12))
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV).eval()
    ei = _graph(31, n_nodes=37)
    rng = np.random.default_rng(32)
    x = torch.randn(37, 24, requires_grad=True)
    last_update = torch.from_numpy(rng.integers(0, 2_600_000, 37))
    t = torch.from_numpy(rng.integers(0, 2_600_000, 300))
    msg = torch.randn(300, 5)
    dout = torch.randn(37, 24)
    want = ref(x, last_update, ei, t, msg)
    want.backward(dout)
    xd = x.detach().to(DEV).requires_grad_(True)
    out = mine(xd, last_update.to(DEV), ei.to(DEV), t.to(DEV), msg.to(DEV))
    out.backward(dout.to(DEV))
    _close(out, want, FWD_TOL, "gnn 24/12/5 out")
    _close(xd.grad, x.grad, GRAD_TOL, "gnn 24/12/5 dx")
    _grads_close(mine, ref, "gnn 24/12/5")


def test_transformer_conv_dropout_in_training():
    from tgnx.nn import TransformerConv
    torch.manual_seed(5)
    ei = _graph(6).to(DEV)
    x, ea = torch.randn(60, 100, device=DEV), torch.randn(300, 272, device=DEV)
    conv = TransformerConv(100, 50, heads=2, dropout=0.1, edge_dim=272).to(DEV).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(x, ei, ea)
    conv.eval()(x, ei, ea)
    conv0 = TransformerConv(100, 50, heads=2, dropout=0.0, edge_dim=272).to(DEV).train()
    conv0(x, ei, ea).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in conv0.parameters())


# ------------------------------------------------------------------ one composed TGN step
D_MSG, D_MEM, N_NODES, N_STORE, B = 172, 100, 50, 120, 40
WIKI = dict(d_msg=D_MSG, d_mem=D_MEM, d_time=D_MEM, n_nodes=N_NODES)
SMALL = dict(d_msg=5, d_mem=24, d_time=12, n_nodes=37)      # memory 24, time 12, raw message 5, 37 nodes


def _tgn_data(seed, dims=WIKI):
    D_MSG, D_MEM, N_NODES = dims["d_msg"], dims["d_mem"], dims["n_nodes"]
    rng = np.random.default_rng(seed)
    d = dict(
        memory=torch.randn(N_NODES, D_MEM, generator=torch.Generator().manual_seed(seed)) * 0.5,
        last_update=torch.from_numpy(rng.integers(0, 1_000_000, N_NODES)),
        s_src=torch.from_numpy(rng.integers(0, N_NODES, N_STORE)),
        s_dst=torch.from_numpy(rng.integers(0, N_NODES, N_STORE)),
        s_raw=torch.from_numpy(rng.standard_normal((N_STORE, D_MSG)).astype(np.float32)),
        src=torch.from_numpy(rng.integers(0, N_NODES, B)),
        pos=torch.from_numpy(rng.integers(0, N_NODES, B)),
        neg=torch.from_numpy(rng.integers(0, N_NODES, B)),
    )
    d["s_t"] = d["last_update"][d["s_src"]] + torch.from_numpy(rng.integers(0, 1_600_000, N_STORE))
    # ring edges: up to 10 per node, 6 on average (~300)
    deg = rng.integers(2, 11, N_NODES)
    e_dst = np.repeat(np.arange(N_NODES), deg)
    E = e_dst.shape[0]
    perm = rng.permutation(E)
    d["edge_index"] = torch.from_numpy(np.stack([rng.integers(0, N_NODES, E)[perm], e_dst[perm]]))
    d["e_t"] = torch.from_numpy(rng.integers(0, 2_600_000, E))
    d["e_msg"] = torch.from_numpy(rng.standard_normal((E, D_MSG)).astype(np.float32))
    if dims is not WIKI:
        # the hub / empty-node construction of _graph: node 7 gathers 150 stored messages and 150 ring edges, node 11
        # sends no stored message and has no incoming edge
        n = d["s_src"].numel()
        d["s_src"] = torch.cat([torch.where(d["s_src"] == 11, (d["s_src"] + 1) % N_NODES, d["s_src"]),
                                torch.full((150,), 7)])
        d["s_dst"] = torch.cat([d["s_dst"], torch.from_numpy(rng.integers(0, N_NODES, 150))])
        d["s_raw"] = torch.cat([d["s_raw"], torch.from_numpy(rng.standard_normal((150, D_MSG)).astype(np.float32))])
        d["s_t"] = torch.cat([d["s_t"], d["last_update"][7] + torch.from_numpy(rng.integers(0, 1_600_000, 150))])
        assert d["s_src"].numel() == n + 150 and int((d["s_src"] == 11).sum()) == 0
        d["edge_index"] = _graph(seed, n_nodes=N_NODES, n_edges=E)
        assert int((d["edge_index"][1] == 7).sum()) == 150 and int((d["edge_index"][1] == 11).sum()) == 0
    return d


def _tgn_loss(m, d):
    """TGNMemory._get_updated_memory + gnn + link_pred (memory_module.py:152-207, pyg_epoch_utils.py:106-137) over
    every node, from explicit tensors; `m` holds the modules of either side."""
    t_rel = (d["s_t"] - d["last_update"][d["s_src"]]).to(torch.float32)
    msg = m["msg"](d["memory"][d["s_src"]], d["memory"][d["s_dst"]], d["s_raw"], m["time_enc"](t_rel))
    aggr = m["aggr"](msg, d["s_src"], d["s_t"], d["memory"].size(0))
    z = m["cell"](aggr, d["memory"])
    z = m["gnn"](z, d["last_update"], d["edge_index"], d["e_t"], d["e_msg"])
    pos, neg = m["pred"](z[d["src"]], z[d["pos"]]), m["pred"](z[d["src"]], z[d["neg"]])
    bce = torch.nn.functional.binary_cross_entropy
    return bce(pos, torch.ones_like(pos)) + bce(neg, torch.zeros_like(neg))


class _Fn(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, *a):
        return self.fn(*a)


def _ref_modules(aggr, cell, dims=WIKI):
    from oracle import tgn_ref as R
    D_MSG, D_MEM = dims["d_msg"], dims["d_mem"]
    te = R.RefTimeEncoder(dims["d_time"])
    in_dim = D_MSG + 2 * D_MEM + dims["d_time"]
    return torch.nn.ModuleDict(dict(
        time_enc=te, msg=_Fn(R.identity_message),
        aggr=_Fn(R.last_aggregate if aggr == "last" else R.mean_aggregate),
        cell=(torch.nn.GRUCell if cell == "gru" else torch.nn.RNNCell)(in_dim, D_MEM),
        gnn=R.RefGraphAttentionEmbedding(D_MEM, D_MEM, D_MSG, te, dropout=0.0), pred=R.RefLinkPredictor(D_MEM)))


def _gpu_modules(aggr, cell, dims=WIKI):
    from tgnx import nn as T
    D_MSG, D_MEM = dims["d_msg"], dims["d_mem"]
    te = T.TimeEncoder(dims["d_time"])
    msg = T.IdentityMessage(D_MSG, D_MEM, dims["d_time"])
    return torch.nn.ModuleDict(dict(
        time_enc=te, msg=msg, aggr=T.LastAggregator() if aggr == "last" else T.MeanAggregator(),
        cell=T.MemoryCell(msg.out_channels, D_MEM, cell),
        gnn=T.GraphAttentionEmbedding(D_MEM, D_MEM, D_MSG, te, dropout=0.0), pred=T.LinkPredictor(D_MEM)))


def _step_and_compare(ref, mine, loss_fn, d, what):
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV)
    dd = {k: v.to(DEV) for k, v in d.items()}
    ref.train(), mine.train()
    opt_r, opt_m = torch.optim.Adam(ref.parameters(), lr=LR, eps=ADAM_EPS), torch.optim.Adam(mine.parameters(), lr=LR,
                                                                                              eps=ADAM_EPS)
    want = loss_fn(ref, d)
    want.backward()
    got = loss_fn(mine, dd)
    got.backward()
    _close(got, want, FWD_TOL, f"{what} loss")
    _grads_close(mine, ref, what)
    ref_grads = {n: p.grad.clone() for n, p in ref.named_parameters()}
    before = {n: p.detach().clone() for n, p in mine.named_parameters()}
    opt_r.step(), opt_m.step()
    refs = dict(ref.named_parameters())
    for n, p in mine.named_parameters():
        if float(ref_grads[n].abs().max()) > 0:
            assert not torch.equal(p.detach(), before[n]), n        # the optimizer reached the parameter
        _adam_close(p, refs[n], ref_grads[n], f"{what} {n} after Adam")
    return ref, mine


@pytest.mark.parametrize("aggr,cell", [("last", "gru"), ("mean", "gru"), ("last", "rnn")])
def test_composed_tgn_step_matches_oracle_composition(aggr, cell):
    torch.manual_seed(10)
    d = _tgn_data(11)
    ref, mine = _ref_modules(aggr, cell), _gpu_modules(aggr, cell)
    assert mine["gnn"].time_enc is mine["time_enc"]
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    _step_and_compare(ref, mine, _tgn_loss, d, f"tgn {aggr} {cell}")


@pytest.mark.parametrize("aggr,cell", [("last", "gru"), ("mean", "gru"), ("last", "rnn"), ("mean", "rnn")])
def test_composed_tgn_step_other_widths_matches_oracle_composition(aggr, cell):
    """Memory 24, time 12, raw message 5 on 37 nodes: a message width of 65, a hub with 150 messages and edges."""
    torch.manual_seed(40)
    d = _tgn_data(41, SMALL)
    ref, mine = _ref_modules(aggr, cell, SMALL), _gpu_modules(aggr, cell, SMALL)
    assert mine["msg"].out_channels == 5 + 2 * 24 + 12
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    _step_and_compare(ref, mine, _tgn_loss, d, f"tgn 24/12/5 {aggr} {cell}")


def test_shared_time_encoder_gets_both_paths_gradients():
    """time_enc feeds the messages and the embedding's edge attributes: its gradient is the sum of the two."""
    torch.manual_seed(12)
    d = {k: v.to(DEV) for k, v in _tgn_data(13).items()}
    mine = _gpu_modules("last", "gru").to(DEV)
    te = mine["time_enc"]
    _tgn_loss(mine, d).backward()
    both = [p.grad.clone() for p in te.parameters()]
    parts = []
    for frozen in ("gnn", "msg"):                                    # cut one use of time_enc at a time
        for p in te.parameters():
            p.grad = None
        m = dict(mine.items())
        cut = _Fn(lambda t, _te=te: _te(t).detach())
        if frozen == "gnn":
            gnn = mine["gnn"]
            m["gnn"] = _Fn(lambda x, lu, ei, t, msg, _g=gnn, _c=cut: _g.conv(
                x, ei, torch.cat([_c((lu[ei[0]] - t).to(x.dtype)), msg], dim=-1)))
        else:
            m["time_enc"] = cut
        _tgn_loss(m, d).backward()
        parts.append([p.grad.clone() for p in te.parameters()])
    for b, p0, p1, name in zip(both, parts[0], parts[1], ("weight", "bias")):
        assert float(p0.abs().max()) > 0 and float(p1.abs().max()) > 0
        _close(b, (p0 + p1).cpu(), GRAD_TOL, f"time_enc.{name} = message path + embedding path")


# ------------------------------------------------------------------ one composed JODIE step
def _jodie_loss(m, d):
    """JODIE: RNN memory update from the aggregated messages, the time projection of the memory to the query time
    (emb_module.py:48-50), LinkPredictor."""
    t_rel = (d["s_t"] - d["last_update"][d["s_src"]]).to(torch.float32)
    msg = m["msg"](d["memory"][d["s_src"]], d["memory"][d["s_dst"]], d["s_raw"], m["time_enc"](t_rel))
    z = m["cell"](m["aggr"](msg, d["s_src"], d["s_t"], d["memory"].size(0)), d["memory"])
    z = m["emb"](z, d["last_update"], d["q_t"])
    pos, neg = m["pred"](z[d["src"]], z[d["pos"]]), m["pred"](z[d["src"]], z[d["neg"]])
    bce = torch.nn.functional.binary_cross_entropy
    return bce(pos, torch.ones_like(pos)) + bce(neg, torch.zeros_like(neg))


class _RefTimeEmbedding(torch.nn.Module):
    """emb_module.py:32-52 restated inline (plain torch)."""

    def __init__(self, out_channels):
        super().__init__()
        self.embedding_layer = torch.nn.Linear(1, out_channels)

    def forward(self, x, last_update, t):
        rel_t = last_update - t
        return x * (1 + self.embedding_layer(rel_t.to(x.dtype).unsqueeze(1)))


def _jodie_step(seed, dims, what):
    from oracle import tgn_ref as R
    from tgnx import nn as T
    D_MSG, D_MEM, D_TIME, N_NODES = dims["d_msg"], dims["d_mem"], dims["d_time"], dims["n_nodes"]
    torch.manual_seed(seed)
    d = _tgn_data(seed + 1, dims)
    # query times shortly after each node's last update (JODIE normalises time: rel_t of order 1)
    d["q_t"] = d["last_update"].float() + torch.rand(N_NODES) * 3.0
    in_dim = D_MSG + 2 * D_MEM + D_TIME
    ref = torch.nn.ModuleDict(dict(time_enc=R.RefTimeEncoder(D_TIME), msg=_Fn(R.identity_message),
                                   aggr=_Fn(R.last_aggregate), cell=torch.nn.RNNCell(in_dim, D_MEM),
                                   emb=_RefTimeEmbedding(D_MEM), pred=R.RefLinkPredictor(D_MEM)))
    mine = torch.nn.ModuleDict(dict(time_enc=T.TimeEncoder(D_TIME), msg=T.IdentityMessage(D_MSG, D_MEM, D_TIME),
                                    aggr=T.LastAggregator(), cell=T.MemoryCell(in_dim, D_MEM, "rnn"),
                                    emb=T.TimeEmbedding(D_MEM, D_MEM), pred=T.LinkPredictor(D_MEM)))
    torch.nn.init.normal_(ref["emb"].embedding_layer.weight, 0.0, 1.0)   # TimeEmbedding's initialisation
    torch.nn.init.normal_(ref["emb"].embedding_layer.bias, 0.0, 1.0)
    _step_and_compare(ref, mine, _jodie_loss, d, what)


def test_composed_jodie_step_matches_torch_restatement():
    _jodie_step(20, WIKI, "jodie")


def test_composed_jodie_step_other_widths_matches_torch_restatement():
    """Memory 24, time 12, raw message 5 on 37 nodes, node 7 a hub of 150 stored messages, node 11 without any."""
    _jodie_step(50, SMALL, "jodie 24/12/5")
