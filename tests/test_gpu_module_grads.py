"""GPU parity of the trainable per-operator layer (csrc/tgnx_ops_bwd.hip through torch.ops.tgnx and the autograd
functions of tgnx/ops.py) against torch CPU autograd of the matching oracle / torch module:

  col_sum                      x.sum(0), incl. no rows, one element, a row-strided view, > 1 row chunk; 1e-4
  memory_cell (gru, rnn)       torch.nn.GRUCell / RNNCell: h' 2e-5; dx, dh, dW_ih, dW_hh, db_ih, db_hh 1e-4
  link_predictor               RefLinkPredictor (sigmoid) and RefEdgePredictor (logits, `tile` pairing): dz_src is
                               the tile-summed gradient; 2e-5 / 1e-4
  time_encode                  RefTimeEncoder with wiki-sized integer timestamps; out 2e-5, dw / db 1e-4
  time_embedding               x (1 + w rel_t + b) written out in torch; 2e-5 / 1e-4
  aggregate_last / _mean       gradient through oracle last_aggregate (BIT-EXACT: a scatter) / mean_aggregate (1e-4)
  linear                       torch.nn.Linear, 2e-5 / 1e-4

Errors are max |a - b| relative to max(|b|, 1) of the reference tensor (module_ref.close); the
tolerances cover reassociation only (MFMA GEMM / fixed-order column sums vs torch's CPU order).  Every backward
op is bit-identical when run twice; a non-contiguous or host tensor raises RuntimeError."""
import numpy as np
import pytest
import torch

from module_ref import close as _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = 2e-5, 1e-4


def _ops():
    from tgnx import ops
    return ops.load()


def _dev(x, grad=False):
    return x.detach().to(DEV).requires_grad_(grad)


# ------------------------------------------------------------------ col_sum
@pytest.mark.parametrize("M,N", [(0, 100), (1, 1), (65, 100), (1000, 300)])
def test_col_sum_matches_and_repeats(M, N):
    ns = _ops()
    torch.manual_seed(M + N)
    x = torch.randn(M, N)
    got = ns.col_sum(x.to(DEV))
    _close(got, x.sum(0), GRAD_TOL, f"col_sum {M}x{N}")
    assert torch.equal(got, ns.col_sum(x.to(DEV)))


def test_col_sum_row_strided_view():
    ns = _ops()
    torch.manual_seed(1)
    wide = torch.randn(300, 172)
    view = wide.to(DEV)[:, 36:136]                            # ldx 172 > N 100
    assert not view.is_contiguous()
    _close(ns.col_sum(view), wide[:, 36:136].sum(0), GRAD_TOL, "col_sum ldx>N")
    with pytest.raises(RuntimeError):
        ns.col_sum(wide.to(DEV).t())                          # unit stride along the rows: rejected
    with pytest.raises(RuntimeError):
        ns.col_sum(wide)                                      # host tensor


# ------------------------------------------------------------------ memory cell
def _cell_case(cell, M, d_in, D, bias=True):
    torch.manual_seed(M * 7 + d_in)
    mod = (torch.nn.GRUCell if cell == "gru" else torch.nn.RNNCell)(d_in, D, bias=bias)
    x, h = torch.randn(M, d_in, requires_grad=True), torch.randn(M, D, requires_grad=True)
    dout = torch.randn(M, D)
    want = mod(x, h)
    want.backward(dout)
    return mod, x, h, dout, want


@pytest.mark.parametrize("cell", ["gru", "rnn"])
@pytest.mark.parametrize("M,d_in,D", [(1, 472, 100), (65, 472, 100), (300, 472, 100), (3, 5, 8)])
def test_memory_cell_grads_match_torch_cell(cell, M, d_in, D):
    from tgnx.ops import memory_cell
    mod, x, h, dout, want = _cell_case(cell, M, d_in, D)
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")

    def run():
        leaves = [_dev(x, True), _dev(h, True)] + [_dev(getattr(mod, n), True) for n in names]
        out = memory_cell(*leaves, cell)
        out.backward(dout.to(DEV))
        return out, leaves
    out, leaves = run()
    _close(out, want, FWD_TOL, f"{cell} h'")
    for got, ref, n in zip(leaves, [x, h] + [getattr(mod, n) for n in names], ("x", "h") + names):
        _close(got.grad, ref.grad, GRAD_TOL, f"{cell} M={M} d{n}")
    _, again = run()
    for a, b in zip(leaves, again):
        assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("cell", ["gru", "rnn"])
def test_memory_cell_without_biases_and_frozen_inputs(cell):
    from tgnx.ops import memory_cell
    mod, x, h, dout, want = _cell_case(cell, 65, 20, 12, bias=False)
    xd, hd = _dev(x, False), _dev(h, True)
    wi, wh = _dev(mod.weight_ih, True), _dev(mod.weight_hh, False)
    out = memory_cell(xd, hd, wi, wh, None, None, cell)
    out.backward(dout.to(DEV))
    _close(out, want, FWD_TOL, "h' no bias")
    assert xd.grad is None and wh.grad is None                # requires_grad=False: no gradient is produced
    _close(hd.grad, h.grad, GRAD_TOL, "dh")
    _close(wi.grad, mod.weight_ih.grad, GRAD_TOL, "dW_ih")
    # the op itself: skipped gradients come back empty
    outs = _ops().gru_update_bwd(dout.to(DEV), xd, hd.detach(), wi.detach(), wh, None, None,
                                 0 if cell == "gru" else 1, [0, 1, 0, 0, 0, 0])
    assert [o.numel() > 0 for o in outs] == [False, True, False, False, False, False]
    assert torch.equal(outs[1], hd.grad)


# ------------------------------------------------------------------ link predictor
@pytest.mark.parametrize("sigmoid", [True, False])
@pytest.mark.parametrize("n_src,k", [(1, 1), (64, 1), (64, 7)])
def test_link_predictor_grads_match_oracle(sigmoid, n_src, k):
    from oracle.tgn_ref import RefLinkPredictor
    from oracle.tgnn_ref import RefEdgePredictor
    from tgnx.ops import link_predictor
    torch.manual_seed(n_src * 10 + k)
    D, M = 100, n_src * k
    zs, zd = torch.randn(n_src, D, requires_grad=True), torch.randn(M, D, requires_grad=True)
    dout = torch.randn(M, 1)
    if k == 1:
        lp = RefLinkPredictor(D)
        params = [lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias, lp.lin_final.weight,
                  lp.lin_final.bias]
        h = (lp.lin_src(zs) + lp.lin_dst(zd)).relu()
        want = lp.lin_final(h)
    else:                                                     # the eval `tile` pairing (model_utils.py:190)
        ep = RefEdgePredictor(D, D)
        params = [ep.src_fc.weight, ep.src_fc.bias, ep.dst_fc.weight, ep.dst_fc.bias, ep.out_fc.weight,
                  ep.out_fc.bias]
        _, want = ep(zs, zd[:n_src], zd, neg_samples=k)
    if sigmoid:
        want = want.sigmoid()
    if k == 1 and sigmoid:
        assert torch.equal(want, lp(zs, zd))                  # the module's own forward
    want.backward(dout)

    def run():
        leaves = [_dev(zs, True), _dev(zd, True)] + [_dev(p, True) for p in params]
        out = link_predictor(*leaves, sigmoid=sigmoid)
        out.backward(dout.to(DEV))
        return out, leaves
    out, leaves = run()
    _close(out, want, FWD_TOL, "pred out")
    names = ("z_src", "z_dst", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out")
    for got, ref, n in zip(leaves, [zs, zd] + params, names):
        _close(got.grad, ref.grad, GRAD_TOL, f"pred d{n} n_src={n_src} k={k} sig={sigmoid}")
    _, again = run()
    for a, b in zip(leaves, again):
        assert torch.equal(a.grad, b.grad)
    # frozen embeddings: no gradient for them
    fz = [_dev(zs, False), _dev(zd, False)] + [_dev(p, True) for p in params]
    link_predictor(*fz, sigmoid=sigmoid).backward(dout.to(DEV))
    assert fz[0].grad is None and fz[1].grad is None
    assert torch.equal(fz[2].grad, leaves[2].grad) and torch.equal(fz[7].grad, leaves[7].grad)


# ------------------------------------------------------------------ time encoder / time embedding
def _wiki_t(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2_600_000, n)).float()


@pytest.mark.parametrize("n", [0, 1, 65, 2000])
def test_time_encode_matches_ref_time_encoder(n):
    from oracle.tgn_ref import RefTimeEncoder
    from tgnx.ops import time_encode
    torch.manual_seed(n)
    D = 100
    enc = RefTimeEncoder(D)
    t = _wiki_t(n, n)
    dout = torch.randn(n, D)
    want = enc(t)
    want.backward(dout)

    def run():
        w, b = _dev(enc.lin.weight, True), _dev(enc.lin.bias, True)
        out = time_encode(t.to(DEV), w, b)
        out.backward(dout.to(DEV))
        return out, w, b
    out, w, b = run()
    _close(out, want, FWD_TOL, f"time_encode n={n}")
    _close(w.grad, enc.lin.weight.grad, GRAD_TOL, f"time_encode dw n={n}")
    _close(b.grad, enc.lin.bias.grad, GRAD_TOL, f"time_encode db n={n}")
    _, w2, b2 = run()
    assert torch.equal(w.grad, w2.grad) and torch.equal(b.grad, b2.grad)


@pytest.mark.parametrize("n", [0, 1, 65, 2000])
def test_time_embedding_matches_formula(n):
    from tgnx.ops import time_embedding
    torch.manual_seed(n + 1)
    D = 100
    lin = torch.nn.Linear(1, D)
    x = torch.randn(n, D, requires_grad=True)
    rel_t = -torch.rand(n) * 50.0                             # last_update - t <= 0, JODIE's scale after normalising
    dout = torch.randn(n, D)
    want = x * (1 + lin(rel_t.unsqueeze(1)))                  # emb_module.py:48-50
    want.backward(dout)

    def run(x_grad=True):
        xd, w, b = _dev(x, x_grad), _dev(lin.weight, True), _dev(lin.bias, True)
        out = time_embedding(xd, rel_t.to(DEV), w, b)
        out.backward(dout.to(DEV))
        return out, xd, w, b
    out, xd, w, b = run()
    _close(out, want, FWD_TOL, f"time_embedding n={n}")
    _close(xd.grad, x.grad, GRAD_TOL, "time_embedding dx")
    _close(w.grad, lin.weight.grad, GRAD_TOL, "time_embedding dw")
    _close(b.grad, lin.bias.grad, GRAD_TOL, "time_embedding db")
    _, x2, w2, b2 = run(x_grad=False)
    assert x2.grad is None and torch.equal(w.grad, w2.grad) and torch.equal(b.grad, b2.grad)


# ------------------------------------------------------------------ aggregators
def _agg_case(rng, n, dim, dim_size):                         # test_gpu_module_ops._agg_case, int64 t
    index = torch.from_numpy(rng.integers(0, dim_size, n))
    if n:
        index[: n // 4] = min(3, dim_size - 1)                # a hub row (250 messages at n = 1000)
    t = torch.from_numpy(rng.integers(0, 20, n))              # many ties
    return torch.randn(n, dim), index, t


@pytest.mark.parametrize("n,dim,dim_size", [(1000, 472, 300), (5, 7, 50), (0, 16, 10)])
def test_aggregator_grads_match_oracle(n, dim, dim_size):
    from oracle.tgn_ref import last_aggregate, mean_aggregate
    from tgnx.ops import aggregate_last, aggregate_mean
    rng = np.random.default_rng(n + dim)
    torch.manual_seed(n + dim)
    msg, index, t = _agg_case(rng, n, dim, dim_size)
    dout = torch.randn(dim_size, dim)
    for name, ref_fn, fn, tol in (("last", last_aggregate, lambda m: aggregate_last(m, index.to(DEV), t.to(DEV), dim_size), 0.0),
                                  ("mean", mean_aggregate, lambda m: aggregate_mean(m, index.to(DEV), dim_size), GRAD_TOL)):
        leaf = msg.clone().requires_grad_(True)
        want = ref_fn(leaf, index, t, dim_size)
        want.backward(dout)
        want_grad = leaf.grad if leaf.grad is not None else torch.zeros_like(msg)
        grads = []
        for _ in range(2):
            md = _dev(msg, True)
            out = fn(md)
            assert torch.equal(out.cpu(), want.detach())      # the forward stays bit-exact
            out.backward(dout.to(DEV))
            grads.append(md.grad)
        assert torch.equal(grads[0], grads[1])
        if tol == 0.0:
            assert torch.equal(grads[0].cpu(), want_grad), name
        else:
            _close(grads[0], want_grad, tol, f"{name} dmsg n={n}")


# ------------------------------------------------------------------ linear
@pytest.mark.parametrize("M,d_in,d_out", [(1, 100, 100), (300, 272, 100)])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_grads_match_nn_linear(M, d_in, d_out, bias):
    from tgnx.ops import linear
    torch.manual_seed(M + d_in)
    lin = torch.nn.Linear(d_in, d_out, bias=bias)
    x = torch.randn(M, d_in, requires_grad=True)
    dout = torch.randn(M, d_out)
    want = lin(x)
    want.backward(dout)

    def run():
        xd, w = _dev(x, True), _dev(lin.weight, True)
        b = _dev(lin.bias, True) if bias else None
        out = linear(xd, w, b)
        out.backward(dout.to(DEV))
        return out, xd, w, b
    out, xd, w, b = run()
    _close(out, want, FWD_TOL, "linear out")
    _close(xd.grad, x.grad, GRAD_TOL, "linear dx")
    _close(w.grad, lin.weight.grad, GRAD_TOL, "linear dW")
    if bias:
        _close(b.grad, lin.bias.grad, GRAD_TOL, "linear db")
    _, x2, w2, b2 = run()
    assert torch.equal(xd.grad, x2.grad) and torch.equal(w.grad, w2.grad)
    assert not bias or torch.equal(b.grad, b2.grad)


# ------------------------------------------------------------------ tensor checks
def test_backward_ops_reject_host_and_non_contiguous_tensors():
    ns = _ops()
    g = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    M, d, D = 4, 6, 8
    good = dict(dh=g(M, D), x=g(M, d), h=g(M, D), wi=g(3 * D, d), wh=g(3 * D, D))
    need = [1] * 6
    ns.gru_update_bwd(good["dh"], good["x"], good["h"], good["wi"], good["wh"], None, None, 0, need)
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.gru_update_bwd(g(D, M).t(), good["x"], good["h"], good["wi"], good["wh"], None, None, 0, need)
    with pytest.raises(RuntimeError, match="device"):
        ns.gru_update_bwd(good["dh"].cpu(), good["x"], good["h"], good["wi"], good["wh"], None, None, 0, need)
    with pytest.raises(RuntimeError):
        ns.gru_update_bwd(good["dh"], good["x"], good["h"], good["wi"], good["wh"], None, None, 2, need)
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.predictor_bwd(g(M), g(D, M).t(), g(M, D), g(D, D), None, g(D, D), None, g(1, D), g(1), True, [1] * 8)
    with pytest.raises(RuntimeError, match="device"):
        ns.predictor_bwd(g(M).cpu(), g(M, D), g(M, D), g(D, D), None, g(D, D), None, g(1, D), g(1), True, [1] * 8)
    with pytest.raises(RuntimeError, match="device"):
        ns.time_encode(torch.zeros(3), g(D, 1), g(D))
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.time_encode_bwd(g(D, 3).t(), g(3), g(D, 1), g(D))
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.time_embedding(g(D, 3).t(), g(3), g(D, 1), g(D))
    with pytest.raises(RuntimeError, match="device"):
        ns.time_embedding_bwd(g(3, D), g(3, D), g(3).cpu(), g(D, 1), g(D), True)
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.msg_agg_last_bwd(g(D, 5).t(), torch.zeros(5, dtype=torch.long, device=DEV), 3)
    with pytest.raises(RuntimeError, match="device"):
        ns.msg_agg_mean_bwd(g(5, D), torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="outside"):
        ns.msg_agg_mean_bwd(g(5, D), torch.tensor([0, 5, 1], device=DEV))
