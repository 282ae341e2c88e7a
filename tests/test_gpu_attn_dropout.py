"""GPU parity of attention dropout in the per-operator layer (csrc/tgnx_ops.hip attn_fwd / attn_bwd <NR, DROP = true>
via torch.ops.tgnx.edge_attn_drop_fwd / _bwd, tgnx.ops.edge_attention(dropout=) and tgnx.nn.TransformerConv) against
the oracle with the same mask injected (oracle.tgn_ref.transformer_attention(keep=), RefTransformerConv.keep).  The mask
is restated in numpy by tests/dropout_ref.py; the cases and their oracle results come from tests/attn_dropout_cases.py.

Bounds are test_gpu_module_ops.py's for these kernels: out and alpha 2e-5, gradients 1e-4, in module_ref.close's
measure (max |a - b| over max(|b|_max, 1)); the module test uses test_gpu_nn_modules.py's (the same numbers).  Every
parity case prints, beside each figure, the dropout-off error of the same operands on the same run.

MEASURED (MI355X; worst over the 16 (shape, key mode, p) cases, in that measure):
    p = 0.1:      out 2.2e-7, alpha 2.4e-7, dq 5.0e-7, dk 4.4e-7, dv 1.7e-7, de 3.1e-7
    p = 0.5:      out 2.0e-7, alpha 2.4e-7, dq 3.7e-7, dk 5.1e-7, dv 1.6e-7, de 3.0e-7
    dropout off:  out 1.9e-7, alpha 2.4e-7, dq 3.9e-7, dk 3.9e-7, dv 1.6e-7, de 3.2e-7   (same operands, same run)
  The factor inv = 2 at p = 0.5 does not show: the errors are fp32 reassociation, two orders below the bounds.
  TransformerConv, train(), p = 0.1: out 2.6e-7, gradients <= 7.5e-7 (lin_key.bias); rows no destination owns:
  exactly zero, the span's values <= 5.4e-7.
"""
import numpy as np
import pytest
import torch

import attn_dropout_cases as A
import dropout_ref as dr
from module_ref import close as _close
from module_ref import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = A.FWD_TOL, A.GRAD_TOL


def _ops():
    from tgnx import ops
    return ops.load()


def _dev(c, *names):
    return [None if c[n] is None else c[n].to(DEV) for n in names]


def _rel(a, b):
    err, scale = rel_err(a, b)
    return err / scale


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("H,C,with_e,mode,p", A.CASES)
def test_edge_attention_dropout_matches_oracle(H, C, with_e, mode, p):
    from tgnx.ops import edge_attention
    c = A.case(H, C, with_e, mode, p)
    stats = A.assert_not_vacuous(c, p)
    print(f"mask: {stats}")
    names = ("q", "k", "v") + (("e",) if with_e else ())
    dl = [c[n].to(DEV).requires_grad_(True) for n in names]
    indptr, dout = c["indptr"].to(DEV), c["dout"].to(DEV)
    explicit = mode == "explicit"
    out, alpha = edge_attention(dl[0], dl[1], dl[2], dl[3] if with_e else None, indptr, H, dropout=p, seed=A.SEED,
                                stream=A.STREAM, dst_key=c["dkey"].to(DEV) if explicit else None,
                                edge_key=c["ekey"].to(DEV) if explicit else None)
    out.backward(dout)
    # the dropout-off error of the same operands, same run (for the figures only)
    d0 = [c[n].to(DEV).requires_grad_(True) for n in names]
    out0, alpha0 = edge_attention(d0[0], d0[1], d0[2], d0[3] if with_e else None, indptr, H)
    out0.backward(dout)
    want0, want_alpha0, grads0 = A.plain_oracle(H, C, with_e)
    print(f"dropout off: out {_rel(out0, want0):.3e} alpha {_rel(alpha0, want_alpha0):.3e} " +
          " ".join(f"d{n} {_rel(x.grad, g):.3e}" for n, x, g in zip(names, d0, grads0)))
    print(f"dropout {p}: out {_rel(out, c['out']):.3e} alpha {_rel(alpha, c['alpha']):.3e} " +
          " ".join(f"d{n} {_rel(x.grad, g):.3e}" for n, x, g in zip(names, dl, c["grads"])))
    _close(out, c["out"], FWD_TOL, "out")
    _close(alpha, c["alpha"], FWD_TOL, "alpha (before dropout)")
    assert torch.equal(alpha, alpha0), "alpha must be the softmax before dropout, bit for bit"
    assert float(out.detach()[5].abs().max()) == 0.0                  # no edges: PyG's empty aggregation
    for n, got, want in zip(names, dl, c["grads"]):
        _close(got.grad, want, GRAD_TOL, f"d{n}")
    # a (destination, head) that lost every edge: a zero head block, and zero dq for that head
    keep, i = c["keep"], c["i"]
    n_kept = torch.zeros(A.N_DST, H).index_add(0, i, (keep != 0).float())
    lost = (n_kept == 0).to(DEV).repeat_interleave(C, dim=1)          # [n_dst, H*C]
    assert bool((out.detach()[lost] == 0).all()), "a head that lost every edge must be exactly zero"
    assert bool((dl[0].grad[lost] == 0).all()), "dq of a head that lost every edge must be exactly zero"
    dropped = (keep == 0).to(DEV).repeat_interleave(C, dim=1)         # [E, H*C]
    assert bool((dl[2].grad[dropped] == 0).all()), "dv of a dropped (edge, head) must be exactly zero"


# ------------------------------------------------------------------ 2. p = 0
@pytest.mark.parametrize("H,C,with_e", A.SHAPES)
@pytest.mark.parametrize("mode", A.KEY_MODES)
def test_p_zero_gives_the_plain_ops_bits(H, C, with_e, mode):
    ns = _ops()
    c = A.case(H, C, with_e, mode, 0.5)
    q, k, v, e, indptr, dout = _dev(c, "q", "k", "v", "e", "indptr", "dout")
    dk_, ek_ = (c["dkey"].to(DEV), c["ekey"].to(DEV)) if mode == "explicit" else (None, None)
    out0, alpha0 = ns.edge_attn_fwd(q, k, v, e, indptr, H)
    g0 = ns.edge_attn_bwd(dout, q, k, v, e, indptr, alpha0, H)
    out, alpha = ns.edge_attn_drop_fwd(q, k, v, e, indptr, H, 0.0, A.SEED, A.STREAM, dk_, ek_)
    g = ns.edge_attn_drop_bwd(dout, q, k, v, e, indptr, alpha, H, 0.0, A.SEED, A.STREAM, dk_, ek_)
    assert torch.equal(out, out0) and torch.equal(alpha, alpha0)
    for name, a, b in zip(("dq", "dk", "dv", "de"), g, g0):
        assert a.shape == b.shape and torch.equal(a, b), name


# ------------------------------------------------------------------ 3. determinism and key plumbing
@pytest.mark.parametrize("H,C,with_e", A.SHAPES)
@pytest.mark.parametrize("mode", A.KEY_MODES)
def test_two_runs_are_equal_and_a_sub_csr_with_keys_gives_the_same_rows(H, C, with_e, mode):
    """Destinations 100..199 as their own CSR with the original keys: the mask is a function of the keys, not of where a
    row stands, so every output row equals the full call's, bit for bit.  In 'default' mode the full call passes no
    keys and the sub call the original row numbers: the defaults are the row numbers."""
    ns = _ops()
    p = 0.5
    c = A.case(H, C, with_e, mode, p)
    q, k, v, e, indptr, dout = _dev(c, "q", "k", "v", "e", "indptr", "dout")
    dkey, ekey = c["dkey"].to(DEV), c["ekey"].to(DEV)
    full_keys = (dkey, ekey) if mode == "explicit" else (None, None)

    def run(q, k, v, e, indptr, dout, dk_, ek_):
        out, alpha = ns.edge_attn_drop_fwd(q, k, v, e, indptr, H, p, A.SEED, A.STREAM, dk_, ek_)
        return (out, alpha) + tuple(ns.edge_attn_drop_bwd(dout, q, k, v, e, indptr, alpha, H, p, A.SEED, A.STREAM,
                                                          dk_, ek_))

    full = run(q, k, v, e, indptr, dout, *full_keys)
    again = run(q, k, v, e, indptr, dout, *full_keys)
    for name, a, b in zip(("out", "alpha", "dq", "dk", "dv", "de"), full, again):
        assert torch.equal(a, b), f"{name}: two runs differ"
    lo, hi = int(c["indptr"][100]), int(c["indptr"][200])
    assert hi - lo > 100
    cut = lambda x: None if x is None else x[lo:hi].contiguous()  # noqa: E731
    sub = run(q[100:200].contiguous(), cut(k), cut(v), cut(e), (indptr[100:201] - lo).contiguous(),
              dout[100:200].contiguous(), dkey[100:200].contiguous(), ekey[lo:hi].contiguous())
    out, alpha, dq, dk, dv, de = full
    want = (out[100:200], alpha[lo:hi], dq[100:200], dk[lo:hi], dv[lo:hi], de[lo:hi] if with_e else de)
    for name, a, b in zip(("out", "alpha", "dq", "dk", "dv", "de"), sub, want):
        assert a.shape == b.shape and torch.equal(a, b), f"{name}: sub-CSR rows differ from the full call's"
    # and the keys matter: other edge keys give another output
    other = ns.edge_attn_drop_fwd(q, k, v, e, indptr, H, p, A.SEED, A.STREAM, full_keys[0], ekey + (1 << 33))[0]
    assert not torch.equal(other, out)


# ------------------------------------------------------------------ 4. rows no destination owns
def _nan_fill(shapes, copies=4):
    """As test_gpu_module_widths.py: fill the allocator's free blocks of these shapes with NaN, so that a row the
    call leaves unwritten reads NaN rather than a lucky zero."""
    torch.cuda.synchronize()
    junk = [torch.full(s, float("nan"), device=DEV) for s in shapes for _ in range(copies)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("H,C", [(2, 50), (8, 32)])
def test_rows_no_destination_owns_are_zero(H, C):
    ns = _ops()
    p, HC, deg = 0.5, H * C, torch.tensor([2, 0, 7, 23])
    E, lo = int(deg.sum()) + 8, 3
    hi = E - 5
    g = torch.Generator().manual_seed(HC)
    indptr = torch.zeros(5, dtype=torch.long)
    indptr[1:] = deg.cumsum(0)
    q, dout = torch.randn(4, HC, generator=g), torch.randn(4, HC, generator=g)
    k, v, e = (torch.randn(E, HC, generator=g) for _ in range(3))
    i = torch.repeat_interleave(torch.arange(4), deg)
    keep = A.keep_mask(A.SEED, A.STREAM, i.numpy(), np.arange(lo, hi), H, p)       # default keys: the rows themselves
    assert 0 < int((keep == 0).sum()) < keep.numel()
    want_out, want_alpha, want = A.oracle(q, k[lo:hi], v[lo:hi], e[lo:hi], i, 4, H, keep, dout)
    qd, kd, vd, ed, dd, ip = (x.to(DEV) for x in (q, k, v, e, dout, indptr + lo))
    outside = torch.ones(E, dtype=torch.bool)
    outside[lo:hi] = False
    _nan_fill([(4, HC), (E, H)])
    out, alpha = ns.edge_attn_drop_fwd(qd, kd, vd, ed, ip, H, p, A.SEED, A.STREAM, None, None)
    _nan_fill([(4, HC), (E, HC)])
    dq, dk, dv, de = ns.edge_attn_drop_bwd(dd, qd, kd, vd, ed, ip, alpha, H, p, A.SEED, A.STREAM, None, None)
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        assert bool((got.cpu()[outside] == 0).all()), f"{name}: rows outside [indptr[0], indptr[n_dst]) are not zero"
    _close(out, want_out, FWD_TOL, "span out")
    _close(alpha[lo:hi], want_alpha, FWD_TOL, "span alpha")
    _close(dq, want[0], GRAD_TOL, "span dq")
    for name, got, w in zip(("dk", "dv", "de"), (dk, dv, de), want[1:4]):
        _close(got[lo:hi], w, GRAD_TOL, f"span {name}")
    # no destinations at all: every edge row is zero
    q0, ip0 = torch.randn(0, HC, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV)
    _nan_fill([(E, H)])
    _, alpha = ns.edge_attn_drop_fwd(q0, kd, vd, ed, ip0, H, p, A.SEED, A.STREAM, None, None)
    _nan_fill([(E, HC)])
    _, dk, dv, de = ns.edge_attn_drop_bwd(q0.clone(), q0, kd, vd, ed, ip0, alpha, H, p, A.SEED, A.STREAM, None, None)
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        assert got.size(0) == E and bool((got == 0).all()), f"{name}: n_dst = 0 must leave every edge row zero"


def test_torch_ops_check_their_key_tensors():
    ns = _ops()
    H, C = 2, 4
    q, k = torch.randn(3, H * C, device=DEV), torch.randn(5, H * C, device=DEV)
    indptr = torch.tensor([0, 2, 2, 5], device=DEV)
    ok_d, ok_e = torch.arange(3, device=DEV), torch.arange(5, device=DEV)
    ns.edge_attn_drop_fwd(q, k, k, None, indptr, H, 0.1, 1, 7, ok_d, ok_e)
    for bad_d, bad_e, _what in [(ok_d.int(), ok_e, "dtype"), (ok_d, ok_e.cpu(), "device"), (ok_d[:2], ok_e, "length"),
                               (ok_d, torch.arange(10, device=DEV)[::2], "contiguous"),
                               (ok_d, ok_e.view(5, 1), "shape")]:
        with pytest.raises(RuntimeError):
            ns.edge_attn_drop_fwd(q, k, k, None, indptr, H, 0.1, 1, 7, bad_d, bad_e)     
    for p, seed in [(1.0, 1), (-0.1, 1), (float("nan"), 1), (0.1, -1)]:
        with pytest.raises(RuntimeError):
            ns.edge_attn_drop_fwd(q, k, k, None, indptr, H, p, seed, 7, None, None)


# ------------------------------------------------------------------ 5. modules
def _graph(seed, n_nodes=60, n_edges=300, hub=7, hub_deg=150, empty=11):
    """test_gpu_nn_modules.py's graph: unsorted edges; node `empty` has no incoming edge and node `hub` has hub_deg."""
    rng = np.random.default_rng(seed)
    others = np.array([i for i in range(n_nodes) if i not in (hub, empty)])
    dst = np.concatenate([np.full(hub_deg, hub), rng.choice(others, n_edges - hub_deg)])
    src = rng.integers(0, n_nodes, n_edges)
    perm = rng.permutation(n_edges)
    return torch.from_numpy(np.stack([src[perm], dst[perm]]))


def _conv_pair(p=0.1):
    from oracle.tgn_ref import RefTransformerConv
    from tgnx.nn import TransformerConv
    torch.manual_seed(0)
    ref = RefTransformerConv(100, 50, 2, p, 272).train()
    mine = TransformerConv(100, 50, heads=2, dropout=p, edge_dim=272)
    mine.load_state_dict(ref.state_dict(), strict=True)
    return ref, mine.to(DEV).train()


def test_transformer_conv_training_dropout_matches_oracle():
    """train(), dropout 0.1, an explicit seed and default keys (destination: the row of x; edge: its column in
    edge_index) against RefTransformerConv with that mask injected: output, dx, dedge_attr and every parameter's
    gradient."""
    ref, mine = _conv_pair()
    seed, ei = 424242, _graph(1)
    x, ea = torch.randn(60, 100, requires_grad=True), torch.randn(300, 272, requires_grad=True)
    dout = torch.randn(60, 100)
    ref.keep = A.keep_mask(seed, 7, ei[1].numpy(), np.arange(300), 2, 0.1)
    dropped = float((ref.keep == 0).double().mean())
    assert 0.05 <= dropped <= 0.2, dropped
    want = ref(x, ei, ea)
    with torch.no_grad():
        keep, ref.keep = ref.keep, torch.ones(300, 2)
        plain = ref(x, ei, ea)
        ref.keep = keep
    assert float((want.detach() - plain).abs().max()) > 100 * FWD_TOL * max(float(plain.abs().max()), 1.0)
    want.backward(dout)
    xd, ead = x.detach().to(DEV).requires_grad_(True), ea.detach().to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="dropout"):
        mine(xd, ei.to(DEV), ead)                                       # no seed known: still raises
    out = mine(xd, ei.to(DEV), ead, seed=seed)
    out.backward(dout.to(DEV))
    _close(out, want, FWD_TOL, "conv out")
    _close(xd.grad, x.grad, GRAD_TOL, "conv dx")
    _close(ead.grad, ea.grad, GRAD_TOL, "conv dedge_attr")
    refs = dict(ref.named_parameters())
    for name, prm in mine.named_parameters():
        assert prm.grad is not None, name
        _close(prm.grad, refs[name].grad, GRAD_TOL, f"conv d{name}")
    # a shuffled edge list whose edge_key names each edge's original column: the same per-edge mask
    perm = torch.from_numpy(np.random.default_rng(9).permutation(300))
    out2 = mine(xd.detach(), ei[:, perm].to(DEV), ead.detach()[perm.to(DEV)], seed=seed, edge_key=perm.to(DEV))
    _close(out2, want, FWD_TOL, "conv out, shuffled edges with their original columns as keys")
    # explicit keys: node ids and event ids, as a TGN loop has them
    n_id = torch.from_numpy(np.random.default_rng(10).permutation(1 << 20)[:60] + (1 << 34))
    e_id = torch.from_numpy(np.random.default_rng(11).permutation(1 << 20)[:300] + (1 << 35))
    ref.keep = A.keep_mask(seed, 7, n_id[ei[1]].numpy(), e_id.numpy(), 2, 0.1)
    with torch.no_grad():
        want3 = ref(x, ei, ea)
    out3 = mine(xd.detach(), ei.to(DEV), ead.detach(), seed=seed, dst_key=n_id.to(DEV), edge_key=e_id.to(DEV))
    _close(out3, want3, FWD_TOL, "conv out, node / event ids as keys")


def test_set_dropout_seed_and_eval():
    from tgnx.nn import TransformerConv
    _, mine = _conv_pair()
    ei = _graph(6).to(DEV)
    x, ea = torch.randn(60, 100, device=DEV), torch.randn(300, 272, device=DEV)
    mine.set_dropout_seed(11)
    a1, a2 = mine(x, ei, ea), mine(x, ei, ea)
    assert not torch.equal(a1, a2), "two consecutive training forwards must draw different masks"
    mine.set_dropout_seed(11)
    assert torch.equal(mine(x, ei, ea), a1), "the first forward after set_dropout_seed(11) must repeat"
    assert torch.equal(mine(x, ei, ea, seed=dr.step_seed(11, 1)), a1)   # the counter's seed is the engine's formula
    conv0 = TransformerConv(100, 50, heads=2, dropout=0.0, edge_dim=272)
    conv0.load_state_dict(mine.state_dict(), strict=True)
    conv0 = conv0.to(DEV).train()
    assert torch.equal(mine.eval()(x, ei, ea), conv0(x, ei, ea)), "eval() must be the dropout-0.0 module bit for bit"
    mine.train().set_dropout_seed(None)
    with pytest.raises(NotImplementedError, match="dropout"):
        mine(x, ei, ea)
