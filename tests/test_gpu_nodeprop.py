"""GPU tests of node property prediction (csrc/tgnx_nodeprop.hip; tgnx.ops.node_predictor / soft_cross_entropy /
ndcg_at_k / node_loss_ndcg; tgnx.nn.NodePredictor; tgnx.nodeprop.train_node / test_node).

  head        forward and backward against the golden captured from the reference's NodePredictor
              (tests/golden/node_pred.npz) and against the float64 restatement (tests/nodeprop_ref.py) on shapes that
              are no multiple of a tile edge, a single row, 1,001 classes (split-K over the classes in dh) and an empty
              batch: logits within FWD_TOL = 2e-5, gradients within GRAD_TOL = 1e-4 in `_close`'s metric (max |a - b|
              over max(|b|, 1), as tests/test_gpu_nn_modules.py);
  row kernel  against the restatement evaluated on the operator's own logits (copied to the CPU): row losses and their
              mean within FWD_TOL, dlogits within GRAD_TOL, ndcg within 1e-12 (the counts are exact integers, the sums at
              most 4,096 float64 terms).  Rows of all-equal logits (W2 = 0), a row with half its scores tied, an all-zero
              target row (loss 0, dlogits 0, ndcg 0), k > C (C = 2, k = 10), k = 3, targets not summing to 1, C a
              multiple of 64, and C = 4,096 (the two-waves-per-workgroup launch);
  repro       two runs of forward + row kernel are bit-identical, a row alone gives the bits it gives inside the batch;
              C = 4,097 and D = 129 are refused with an error;
  composed    GraphAttentionEmbedding -> NodePredictor -> soft_cross_entropy -> Adam against the oracle composition on
              the CPU: gradients at GRAD_TOL, parameters after the step under the first-Adam-step bound of
              tests/test_gpu_nn_modules.py (restated at `_adam_close`);
  loops       60 nodes, 600 events, d = 8, D = 36, ring 10, batch 50, labels from make_labels with C = 7: test_node
              leaves memory, last_update and ring bit for bit as a second engine driven by hand with observe_range /
              embed over label_schedule, and returns that engine's per-group ndcg_at_k; train_node with lr = 0 returns
              test_node's metrics, with lr > 0 it moves only the head: model.state_dict() equals the lr = 0 pass's."""
import numpy as np
import pytest
import torch

import nodeprop_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL, NDCG_TOL = 2e-5, 1e-4, 1e-12
LR, ADAM_EPS = 1e-3, 1e-8
PARAMS = ("lin_node.weight", "lin_node.bias", "out.weight", "out.bias")


def _close(a, b, tol, what=""):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e} tol {tol:g}")
    assert err <= tol * scale, (what, err, scale)


def _adam_close(p_gpu, p_ref, g_ref, what):
    """The first Adam step moves p by lr u(g), u(g) = g / (|g| + eps), ill-conditioned where g ~ 0: the bound on
    |p_gpu - p_ref| is lr times the change of u over [g - δ, g + δ], δ = GRAD_TOL max(|g|_max, 1) (u is monotonic:
    the extremes are at the ends), plus fp32 rounding of p."""
    p_gpu, p_ref, g = p_gpu.detach().double().cpu(), p_ref.detach().double(), g_ref.detach().double()
    delta = GRAD_TOL * max(float(g.abs().max()), 1.0)
    u = lambda x: x / (x.abs() + ADAM_EPS)  # noqa: E731
    bound = LR * torch.maximum((u(g + delta) - u(g)).abs(), (u(g - delta) - u(g)).abs())
    bound = bound + 1e-6 * p_ref.abs().clamp(min=1.0)
    excess = float(((p_gpu - p_ref).abs() - bound).max())
    print(f"{what}: max |dp| {float((p_gpu - p_ref).abs().max()):.3e}, over bound by {excess:.3e}")
    assert excess <= 0.0, (what, excess)


def _head(D, C, seed):
    from tgnx.nn import NodePredictor
    torch.manual_seed(seed)
    return NodePredictor(D, C)


def _targets(M, C, seed):
    """Sparse non-negative targets: 1-8 classes per row, normalised; every fourth row scaled off a unit sum."""
    rng = np.random.default_rng(seed)
    y = np.zeros((M, C), dtype=np.float32)
    for i in range(M):
        nz = rng.choice(C, size=min(C, int(rng.integers(1, 9))), replace=False)
        cnt = rng.integers(1, 6, size=nz.shape[0]).astype(np.float32)
        y[i, nz] = cnt / cnt.sum() * (1.0 if i % 4 else 2.5)
    return y


def _np_params(head):
    sd = {k: v.detach().cpu().numpy() for k, v in head.state_dict().items()}
    return sd["lin_node.weight"], sd["lin_node.bias"], sd["out.weight"], sd["out.bias"]


# ------------------------------------------------------------------ head forward / backward
@pytest.mark.parametrize("M,D,C", [(1, 100, 2), (67, 100, 65), (130, 36, 255), (300, 100, 1001), (0, 100, 65)])
def test_head_forward_backward_matches_restatement(M, D, C):
    rng = np.random.default_rng(M + C)
    head = _head(D, C, 3).to(DEV)
    z = rng.standard_normal((M, D)).astype(np.float32)
    dout = rng.standard_normal((M, C)).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV).requires_grad_(True)
    logits = head(zd)
    assert logits.shape == (M, C)
    logits.backward(torch.from_numpy(dout).to(DEV))
    torch.cuda.synchronize()
    w1, b1, w2, b2 = _np_params(head)
    want, h = R.head_forward(z, w1, b1, w2, b2)
    _close(logits, want, FWD_TOL, "logits")
    g = R.head_backward(dout, z, h, w1, w2)
    _close(zd.grad, g["dz"], GRAD_TOL, "dz")
    for p, key in ((head.lin_node.weight, "dw1"), (head.lin_node.bias, "db1"), (head.out.weight, "dw2"),
                   (head.out.bias, "db2")):
        _close(p.grad, g[key], GRAD_TOL, key)
    if M == 0:
        assert all(not bool(p.grad.any()) for p in head.parameters())
    # inference: no hidden rows kept, the same logits
    with torch.no_grad():
        assert torch.equal(head(zd.detach()), logits.detach())


def test_head_and_loss_match_the_golden(golden):
    from tgnx import ops
    g = golden("node_pred.npz")
    head = _head(100, 65, 0)
    head.load_state_dict({n: torch.from_numpy(g["sd." + n]) for n in PARAMS}, strict=True)
    head = head.to(DEV)
    z = torch.from_numpy(g["z"]).to(DEV).requires_grad_(True)
    logits = head(z)
    loss = ops.soft_cross_entropy(logits, torch.from_numpy(g["y"]).to(DEV))
    loss.backward()
    _close(logits, g["logits"], FWD_TOL, "logits")
    _close(loss, g["loss"], FWD_TOL, "loss")
    _close(z.grad, g["dz"], GRAD_TOL, "dz")
    for n, p in head.named_parameters():
        _close(p.grad, g["grad." + n], GRAD_TOL, "d" + n)


# ------------------------------------------------------------------ the row kernel
def _rows_check(logits, y, k):
    """The raw op on device logits / targets against the restatement on the same logits."""
    from tgnx import ops
    M = logits.shape[0]
    mean, rows, dl, nd = ops.load().node_loss_ndcg(logits, y, ops._cum_on(k, DEV), k, True, True, True)
    torch.cuda.synchronize()
    lh, yh = logits.cpu().numpy(), y.cpu().numpy()
    want_rows, want_dl = R.soft_ce(lh, yh)
    want_nd = R.ndcg_rows(lh, yh, k)
    _close(rows, want_rows, FWD_TOL, "loss rows")
    _close(mean, want_rows.mean(), FWD_TOL, "mean loss")
    _close(dl, want_dl, GRAD_TOL, "dlogits")
    # scale 1 / M: compare the gradient of the loss SUM too, so that the bound does not loosen with M
    _close(dl.double() * M, want_dl * M, GRAD_TOL, "dlogits x M")
    err = float(np.abs(nd.cpu().numpy() - want_nd).max())
    print(f"ndcg@{k}: err {err:.3e}")
    assert nd.dtype == torch.float64 and err <= NDCG_TOL, err
    # the public forms return the same bits
    assert torch.equal(ops.ndcg_at_k(logits, y, k), nd)
    l2 = logits.clone().requires_grad_(True)
    loss, nd2 = ops.node_loss_ndcg(l2, y, k)
    loss.backward()
    assert torch.equal(loss.detach(), mean) and torch.equal(nd2, nd) and torch.equal(l2.grad, dl)
    l3 = logits.clone().requires_grad_(True)
    (ops.soft_cross_entropy(l3, y) * 3.0).backward()               # an incoming gradient other than 1
    _close(l3.grad, want_dl * 3.0, GRAD_TOL, "dlogits, incoming gradient 3")
    return rows, dl, nd


@pytest.mark.parametrize("M,D,C,k", [(67, 100, 65, 10), (67, 100, 65, 3), (5, 100, 2, 10), (300, 100, 1001, 10),
                                     (9, 36, 128, 10), (5, 36, 4096, 10)])
def test_row_kernel_matches_restatement_on_its_own_logits(M, D, C, k):
    head = _head(D, C, 5).to(DEV)
    rng = np.random.default_rng(7 * M + C)
    with torch.no_grad():
        logits = head(torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32)).to(DEV))
        if M > 2:
            logits[1, : C // 2] = float(logits[1, 0])                # a row with half its scores tied
    y = _targets(M, C, M + C)
    if M > 2:
        y[2] = 0.0                                                   # an all-zero target row
        y[1, : max(C // 4, 1)] = 0.5                                 # positive targets inside the tie group
    rows, dl, nd = _rows_check(logits.contiguous(), torch.from_numpy(y).to(DEV), k)
    if M > 2:
        assert float(rows[2]) == 0.0 and not bool(dl[2].any()) and float(nd[2]) == 0.0
        assert int((logits[1] == logits[1, 0]).sum()) >= C // 2
    assert bool(((nd >= 0) & (nd <= 1 + 1e-12)).all())


def test_row_kernel_all_equal_logits():
    """W2 = 0: every class scores b2 (one tie group of C classes), so each positive class gets the mean discount."""
    C, k = 65, 10
    head = _head(100, C, 6).to(DEV)
    with torch.no_grad():
        head.out.weight.zero_()
        head.out.bias.fill_(0.375)
        logits = head(torch.randn(12, 100, device=DEV))
    assert bool((logits == 0.375).all())
    y = torch.from_numpy(_targets(12, C, 9)).to(DEV)
    rows, _, nd = _rows_check(logits, y, k)
    cum = R.ndcg_cum(k)
    yh = y.cpu().double().numpy()
    for i in range(12):
        idcg = (np.sort(yh[i])[::-1][:k] * np.diff(cum)).sum()
        assert abs(float(nd[i]) - yh[i].sum() * cum[k] / C / idcg) <= NDCG_TOL
    _close(rows, np.log(C) * yh.sum(1) , FWD_TOL, "uniform rows: log C x sum y")


def test_bit_identical_runs_and_rows_independent_of_the_batch():
    from tgnx import ops
    M, D, C, k = 300, 100, 1001, 10
    head = _head(D, C, 8).to(DEV)
    z = torch.randn(M, D, device=DEV)
    y = torch.from_numpy(_targets(M, C, 4)).to(DEV)
    cum = ops._cum_on(k, DEV)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            logits = head(z)
        runs.append((logits,) + tuple(ops.load().node_loss_ndcg(logits, y, cum, k, True, True, True)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    logits, _, rows, _, nd = runs[0]
    for lo, hi in ((0, 1), (7, 10), (297, 300)):                     # another grid, other waves: the same bits
        _, r, _, n = ops.load().node_loss_ndcg(logits[lo:hi].contiguous(), y[lo:hi].contiguous(), cum, k, True, False,
                                               True)
        assert torch.equal(r, rows[lo:hi]) and torch.equal(n, nd[lo:hi])


def test_sizes_outside_the_domain_are_refused():
    from tgnx import ops
    ns = ops.load()
    f = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="bad sizes"):
        ns.node_predictor(f(4, 100), f(100, 100), f(100), f(4097, 100), f(4097), False)
    with pytest.raises(RuntimeError, match="bad sizes"):
        ns.node_predictor(f(4, 129), f(129, 129), f(129), f(65, 129), f(65), True)
    with pytest.raises(RuntimeError, match="bad sizes"):
        ns.node_predictor_bwd(f(4, 65), f(4, 129), f(4, 129), f(129, 129), f(65, 129), [1, 1, 1, 1, 1])
    with pytest.raises(RuntimeError, match="bad sizes"):
        ns.node_loss_ndcg(f(4, 4097), f(4, 4097), ops._cum_on(10, DEV), 10, True, True, True)
    with pytest.raises(ValueError, match="k must be"):
        ops.ndcg_at_k(f(4, 7), f(4, 7), 129)
    torch.cuda.synchronize()
    assert float(ops.soft_cross_entropy(f(4, 7), f(4, 7))) == 0.0    # the device is fine afterwards


# ------------------------------------------------------------------ one composed step
class _RefNodePredictor(torch.nn.Module):
    """modules/decoder.py:30-41 restated in plain torch."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.lin_node = torch.nn.Linear(in_dim, in_dim)
        self.out = torch.nn.Linear(in_dim, out_dim)

    def forward(self, x):
        return self.out(self.lin_node(x).relu())


def test_composed_embedding_head_step_matches_oracle_composition():
    from oracle import tgn_ref as O
    from tgnx import nn as T
    from tgnx import ops
    torch.manual_seed(30)
    Dm, dm, N, E, C = 100, 172, 60, 300, 65
    rng = np.random.default_rng(31)
    ref = torch.nn.ModuleDict(dict(gnn=O.RefGraphAttentionEmbedding(Dm, Dm, dm, O.RefTimeEncoder(Dm), dropout=0.0),
                                   head=_RefNodePredictor(Dm, C)))
    mine = torch.nn.ModuleDict(dict(gnn=T.GraphAttentionEmbedding(Dm, Dm, dm, T.TimeEncoder(Dm), dropout=0.0),
                                    head=T.NodePredictor(Dm, C)))
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine = mine.to(DEV)
    d = dict(x=torch.randn(N, Dm), last_update=torch.from_numpy(rng.integers(0, 2_600_000, N)),
             ei=torch.from_numpy(np.stack([rng.integers(0, N, E), rng.integers(0, N, E)])),
             t=torch.from_numpy(rng.integers(0, 2_600_000, E)), msg=torch.randn(E, dm),
             nodes=torch.from_numpy(rng.integers(0, N, 41)), y=torch.from_numpy(_targets(41, C, 32)))
    dd = {k: v.to(DEV) for k, v in d.items()}

    def loss_fn(m, d, ce):
        z = m["gnn"](d["x"], d["last_update"], d["ei"], d["t"], d["msg"])
        return ce(m["head"](z[d["nodes"]]), d["y"])

    ref.train(), mine.train()
    opt_r = torch.optim.Adam(ref.parameters(), lr=LR, eps=ADAM_EPS)
    opt_m = torch.optim.Adam(mine.parameters(), lr=LR, eps=ADAM_EPS)
    want = loss_fn(ref, d, torch.nn.functional.cross_entropy)
    want.backward()
    got = loss_fn(mine, dd, ops.soft_cross_entropy)
    got.backward()
    _close(got, want, FWD_TOL, "composed loss")
    refs = dict(ref.named_parameters())
    assert [n for n, _ in mine.named_parameters()] == list(refs)
    for n, p in mine.named_parameters():
        assert p.grad is not None, n
        _close(p.grad, refs[n].grad, GRAD_TOL, f"composed d{n}")
    assert float(mine["gnn"].conv.lin_query.weight.grad.abs().max()) > 0     # dz reached the embedding
    ref_grads = {n: p.grad.clone() for n, p in refs.items()}
    opt_r.step(), opt_m.step()
    for n, p in mine.named_parameters():
        _adam_close(p, refs[n], ref_grads[n], f"composed {n} after Adam")


# ------------------------------------------------------------------ the loops
N, NEV, d_MSG, D_MEM, B, C_LAB = 60, 600, 8, 36, 50, 7
STATE = ("memory", "last_update", "neighbors", "e_id", "t")
_LOOP = {}


def _loop_setup():
    if not _LOOP:
        from oracle.tgn_ref import RefTGN
        from tgnx.nodeprop import make_labels
        from tgnx.synth import make_stream
        s = make_stream("tgbl-wiki", seed=5, num_events=NEV, num_nodes=N, msg_dim=d_MSG)
        torch.manual_seed(0)
        sd = RefTGN(N, d_MSG, hidden=D_MEM, dropout=0.0).state_dict()
        labels = make_labels(s, C_LAB, (s.t[-1] - s.t[0]) / 6)
        head = _head(D_MEM, C_LAB, 11).to(DEV)
        _LOOP.update(s=s, sd=sd, labels=labels, head_sd={k: v.clone() for k, v in head.state_dict().items()})
    return _LOOP


def _loop_engine():
    from tgnx.sampler import LastNeighborLoader
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    L = _loop_setup()
    s = L["s"]
    model = TGNModel(N, NEV, d_MSG, D_MEM, DEV, ring=10, max_batch=B, max_neg=1, dropout=0.0)
    model.load_reference_state(L["sd"])
    loader = LastNeighborLoader(N, 10, device=DEV)
    eng = TgnEngine(model, loader, dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg),
                    TgnAdam(model, 1e-3), dst_nodes=s.dst_nodes, seed=7)
    eng.reset_state()
    eng._mode_train = False
    model._tgnx_engine = eng                                         # what train() / test() attach
    return model, loader, eng


def _loop_head():
    head = _head(D_MEM, C_LAB, 11).to(DEV)
    head.load_state_dict(_loop_setup()["head_sd"])
    return head


def _state(eng):
    torch.cuda.synchronize()
    m, ld = eng.model, eng.loader
    return dict(memory=m.memory.memory, last_update=m.memory.last_update, neighbors=ld.neighbors, e_id=ld.e_id, t=ld.t)


def test_test_node_equals_a_hand_driven_engine():
    from tgnx import ops
    from tgnx.nodeprop import label_schedule, test_node
    L = _loop_setup()
    labels, head = L["labels"], _loop_head()
    model, loader, eng = _loop_engine()
    out = test_node(model, loader, head, labels, 0, NEV, batch=B, k=10)
    _, _, hand = _loop_engine()
    sched = label_schedule(L["s"].t.astype(np.float32), labels, 0, NEV)
    assert 4 <= len(sched) <= 7 and out["groups"] == len(sched) and out["rows"] == sum(b - a for _, a, b in sched)
    prev, nds, losses = 0, [], []
    with torch.no_grad():
        for r_g, a, b in sched:
            hand.observe_range(prev, r_g, B)
            prev = r_g
            logits = head(hand.embed(labels.node[a:b]))
            y = labels.dense(a, b, DEV)
            nds.append(ops.ndcg_at_k(logits, y, 10))
            losses.append(float(ops.soft_cross_entropy(logits, y)))
        hand.observe_range(prev, NEV, B)
    sa, sb = _state(eng), _state(hand)
    for key in STATE:
        x, y = sa[key], sb[key]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), key
    assert float(sa["memory"].abs().max()) > 0 and loader.cur_e_id == NEV
    assert torch.equal(out["group_ndcg"], torch.stack([n.mean() for n in nds]))
    assert out["ndcg"] == pytest.approx(float(torch.stack([n.mean() for n in nds]).mean()), abs=1e-12)
    assert out["ndcg_rows"] == pytest.approx(float(torch.cat(nds).mean()), abs=1e-12)
    assert out["loss"] == pytest.approx(float(np.mean(losses)), abs=1e-6)
    # two adjacent passes partition the groups and leave the same state as one
    model2, loader2, eng2 = _loop_engine()
    cut = sched[len(sched) // 2][0]
    o1 = test_node(model2, loader2, head, labels, 0, cut, batch=B)
    o2 = test_node(model2, loader2, head, labels, cut, NEV, batch=B)
    assert o1["groups"] + o2["groups"] == out["groups"] and o1["rows"] + o2["rows"] == out["rows"]
    assert torch.equal(torch.cat([o1["group_ndcg"], o2["group_ndcg"]]), out["group_ndcg"])
    for key, x in _state(eng2).items():
        assert torch.equal(x, sa[key]), key


def test_train_node_moves_only_the_head():
    from tgnx.nodeprop import test_node, train_node
    L = _loop_setup()
    labels = L["labels"]
    model, loader, eng = _loop_engine()
    head0 = _loop_head()
    want = test_node(model, loader, head0, labels, 0, NEV, batch=B)
    # lr = 0: the same metrics, from a reset of whatever state the engine was in
    head = _loop_head()
    got = train_node(model, loader, head, torch.optim.Adam(head.parameters(), lr=0.0), labels, 0, NEV, batch=B)
    for key in ("loss", "ndcg", "ndcg_rows", "groups", "rows"):
        assert got[key] == want[key], key
    assert torch.equal(got["group_ndcg"], want["group_ndcg"])
    frozen = {k: v.clone() for k, v in model.state_dict().items()}
    # lr > 0: the head moves, the model does not
    head = _loop_head()
    before = {k: v.clone() for k, v in head.state_dict().items()}
    out = train_node(model, loader, head, torch.optim.Adam(head.parameters(), lr=1e-2), labels, 0, NEV, batch=B,
                     label_batch=16)
    assert out["groups"] == want["groups"] and out["rows"] == want["rows"] and np.isfinite(out["loss"])
    assert all(not torch.equal(v, before[k]) for k, v in head.state_dict().items())
    after = model.state_dict()
    assert set(after) == set(frozen)
    for k2, v in after.items():
        assert torch.equal(v, frozen[k2]), k2
    eng.world = 2
    with pytest.raises(ValueError, match="one device only"):
        train_node(model, loader, head, None, labels, 0, NEV)
    eng.world = 1
