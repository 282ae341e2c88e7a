"""The per-operator layer (torch.ops.tgnx.*, the autograd functions of tgnx/ops.py; csrc/tgnx_ops.hip and
csrc/tgnx_ops_bwd.hip) against a float64 reference (tests/module_ref.py) at the widths, head layouts and row counts
where its kernels change path — what a caller composing "another message function, JODIE, a changed predictor"
runs, beyond the tgbl-wiki shape (D = 100, d_in = 472) of test_gpu_module_ops.py / test_gpu_module_grads.py.

  edge attention   16 (H, C) from (1, 1) to (1, 256): H up to HMAX = 8, H·C at 63..65 / 128 / 129 / 255 / 256 (one,
                   two or four registers per lane), heads that straddle a lane's registers; with and without e;
                   37 destinations of degree [0, 1, 2, 63, 64, 65, 150, ...] (a last block with one live wave), a
                   single destination, and no edge at all; q at scale 1 and 8 (scores up to 90: expf needs the max
                   subtraction).  out / α 2e-5, gradients 1e-4; a destination without edges has out = dq = 0 exactly;
                   α sums to 1 within 1e-6; a degree-1 destination has α = 1 and dq = 0 exactly; backward repeats bit
                   for bit; heads = 9, H·C = 257, H·C not a multiple of heads raise
  rows no destination owns   indptr spanning [3, E - 5) of the E edge rows, and n_dst = 0 with E = 4: α, dk, dv, de are
                   0 there (the allocator's free blocks are NaN-filled first), the span equals the reference on the span
  col_sum          M in 255..513 x N in 1..129 (one chunk vs partials; one strip vs two), a row-strided view
  memory cell      gru / rnn at 7 (M, d_in, D) from (1, 1, 1) to (3, 17, 172), one without biases
  link predictor   D in 1..172 x (n_src, k) in (1, 1), (3, 5), (257, 1), sigmoid on / off, and d_in 20 != D 65; row i
                   pairs with source i mod n_src
  linear, time encoder, time embedding   D in 1..172 x n in 1, 255, 257; linear 257 x 65 -> 129 with / without bias
  time encoder at |w t| up to 2^30   b = 0, so the argument is the float32 product rounded once (numpy reproduces it);
                   against cos / sin of that float32 argument in float64: forward within 2^-23 ABSOLUTE (one float ulp
                   at 1: te_cos claims a double computation rounded once), dw / db 1e-4
  aggregators      dim in 1..129; rows of exactly 63 / 64 / 65 equal-t messages, a unique maximum at the 65th, a tie
                   between the 1st and the 65th, negative int64 t, fp32 t with -0.0 and 0.0 (they tie): forward and
                   argmax bit-exact, last's gradient bit-exact, mean's 1e-4

Tolerances are the project's own (2e-5 forward, 1e-4 gradients; max |a - b| over max(|b|_max, 1)), now against
float64.  test_module_ref_cpu.py holds every input to a tenth of them in plain fp32 CPU arithmetic.  Measured there
(fp32 CPU vs float64, this file's attention sweep, every degree pattern, q x 1 and x 8): worst out / α error 1.6e-6,
worst gradient error 3.1e-6 (an earlier sweep with other draws: 1.4e-6 / 1.7e-6).  Measured on an MI355X, the
kernels vs float64 over this whole file: worst forward error 1.6e-6, worst gradient error 3.3e-6, worst
|sum alpha - 1| 6.9e-7, time encoder at |w t| up to 2^30 3.0e-8 (2^-23 = 1.2e-7)."""
import pytest
import torch

import module_ref as R
from module_ref import FWD_TOL, GRAD_TOL, close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _ops():
    from tgnx import ops
    return ops.load()


def _dev(x, grad=False):
    return None if x is None else x.detach().to(DEV).requires_grad_(grad and x.is_floating_point())


def _run(fn, inputs, dout):
    """fn on device leaves: (out, leaves) after backward."""
    leaves = [_dev(x, True) for x in inputs]
    out = fn(*leaves)
    out.backward(dout.to(DEV))
    return out, leaves


def _check(fn, case, names, what, repeat=True):
    out, leaves = _run(fn, case["inputs"], case["dout"])
    close(out, case["out"], FWD_TOL, f"{what} out")
    for name, leaf, want in zip(names, leaves, case["grads"]):
        if want is not None:
            close(leaf.grad, want, GRAD_TOL, f"{what} d{name}")
    if repeat:
        out2, again = _run(fn, case["inputs"], case["dout"])
        assert torch.equal(out, out2)
        for a, b in zip(leaves, again):
            assert a is None or a.grad is None or torch.equal(a.grad, b.grad), what
    return out, leaves


# ------------------------------------------------------------------ edge attention
@pytest.mark.parametrize("with_e", [True, False])
@pytest.mark.parametrize("H,C", R.ATTN_HC)
def test_edge_attention_widths(H, C, with_e):
    from tgnx.ops import edge_attention
    for pattern in R.ATTN_PATTERNS:
        for s in R.ATTN_Q_SCALES:
            case = R.attn_case(H, C, with_e, pattern, s)
            what = f"attn H={H} C={C} e={int(with_e)} {pattern} q*{s:g}"
            deg = case["deg"]

            def run():
                q, k, v, e, indptr = (_dev(x, True) for x in case["inputs"])
                out, alpha = edge_attention(q, k, v, e, indptr, H)
                out.backward(case["dout"].to(DEV))
                return out, alpha, [q, k, v] + ([e] if with_e else [])
            out, alpha, leaves = run()
            close(out, case["out"], FWD_TOL, f"{what} out")
            close(alpha, case["alpha"], FWD_TOL, f"{what} alpha")
            for name, leaf, want in zip("qkve", leaves, case["grads"]):
                want = want if want is not None else torch.zeros_like(leaf, device="cpu")
                close(leaf.grad, want, GRAD_TOL, f"{what} d{name}")
            # a destination without edges: PyG's empty aggregation, and nothing flows back to its query
            assert float(out.detach()[deg == 0].abs().sum()) == 0.0
            assert float(leaves[0].grad[deg == 0].abs().sum()) == 0.0
            i = torch.repeat_interleave(torch.arange(deg.numel()), deg)
            sums = torch.zeros(deg.numel(), H, dtype=torch.float64).index_add(0, i, alpha.detach().double().cpu())
            if bool((deg > 0).any()):
                off = float((sums[deg > 0] - 1.0).abs().max())
                print(f"{what}: |sum alpha - 1| {off:.3e}")
                assert off <= 1e-6, (what, off)
            one = deg == 1
            assert torch.equal(alpha.detach().cpu()[one[i]], torch.ones(int(one.sum()), H))
            assert float(leaves[0].grad[one].abs().sum()) == 0.0
            _, alpha2, again = run()
            assert torch.equal(alpha, alpha2)
            for a, b in zip(leaves, again):
                assert torch.equal(a.grad, b.grad), what


def test_edge_attention_rejects_sizes_it_has_no_kernel_for():
    from tgnx.ops import edge_attention
    ns = _ops()
    indptr = torch.tensor([0, 2, 3], device=DEV)

    def args(HC):
        return torch.randn(2, HC, device=DEV), torch.randn(3, HC, device=DEV), torch.randn(3, HC, device=DEV)
    for HC, heads in ((18, 9), (257, 1), (10, 3)):              # heads > 8; H·C > 256; H·C not a multiple of heads
        q, k, v = args(HC)
        with pytest.raises(RuntimeError):
            edge_attention(q, k, v, None, indptr, heads)
        with pytest.raises(RuntimeError):
            ns.edge_attn_fwd(q, k, v, k.clone(), indptr, heads)
        with pytest.raises(RuntimeError):
            ns.edge_attn_bwd(torch.randn_like(q), q, k, v, None, indptr, torch.rand(3, heads, device=DEV), heads)
    q, k, v = args(16)                                          # the same call goes through at a size there is
    assert edge_attention(q, k, v, None, indptr, 8)[0].shape == (2, 16)


def _nan_fill(shapes, copies=32):
    """Fill the caching allocator's free blocks with NaN: allocate NaN tensors of the sizes the next call will ask
    for, and free them, so that an output row the call leaves unwritten reads NaN rather than a lucky zero."""
    torch.cuda.synchronize()
    junk = [torch.full(s, float("nan"), device=DEV) for s in shapes for _ in range(copies)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("H,C", [(2, 50), (8, 32)])
def test_edge_attention_rows_no_destination_owns_are_zero(H, C):
    """indptr need not span all E edge rows (the op clamps and accepts any indptr): α and the edge gradients of a row
    outside [indptr[0], indptr[n_dst]) are 0, never uninitialised memory."""
    ns = _ops()
    HC, deg = H * C, torch.tensor([2, 0, 7, 23])
    E, lo = int(deg.sum()) + 8, 3
    hi = E - 5
    g = torch.Generator().manual_seed(HC)
    indptr = torch.zeros(5, dtype=torch.long)
    indptr[1:] = deg.cumsum(0)
    assert int(indptr[-1]) == hi - lo
    q, dout = torch.randn(4, HC, generator=g), torch.randn(4, HC, generator=g)
    k, v, e = (torch.randn(E, HC, generator=g) for _ in range(3))
    fn = R.attn_ref(H)
    want_out, want = R.run_ref(fn, (q, k[lo:hi], v[lo:hi], e[lo:hi], indptr), dout, torch.float64)
    qd, kd, vd, ed, dd, ip = (x.to(DEV) for x in (q, k, v, e, dout, indptr + lo))
    outside = torch.ones(E, dtype=torch.bool)
    outside[lo:hi] = False
    _nan_fill([(4, HC), (E, H)])
    out, alpha = ns.edge_attn_fwd(qd, kd, vd, ed, ip, H)
    _nan_fill([(4, HC), (E, HC)])
    dq, dk, dv, de = ns.edge_attn_bwd(dd, qd, kd, vd, ed, ip, alpha, H)
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        rows = got.cpu()[outside]
        print(f"{name} outside the span: {int(torch.isnan(rows).sum())} NaN, {int((rows != 0).sum())} non-zero of "
              f"{rows.numel()}")
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        assert bool((got.cpu()[outside] == 0).all()), f"{name}: rows outside [indptr[0], indptr[n_dst]) are not zero"
    close(out, want_out, FWD_TOL, "span out")
    close(alpha[lo:hi], fn.alpha, FWD_TOL, "span alpha")
    close(dq, want[0], GRAD_TOL, "span dq")
    for name, got, w in zip(("dk", "dv", "de"), (dk, dv, de), want[1:4]):
        close(got[lo:hi], w, GRAD_TOL, f"span {name}")
    # without e: de comes back empty, the rest keeps the guarantee
    _nan_fill([(4, HC), (E, H)])
    _, alpha = ns.edge_attn_fwd(qd, kd, vd, None, ip, H)
    _nan_fill([(4, HC), (E, HC)])
    _, dk, dv, de = ns.edge_attn_bwd(dd, qd, kd, vd, None, ip, alpha, H)
    assert de.numel() == 0
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv)):
        assert bool((got.cpu()[outside] == 0).all()), f"{name} (no e): rows outside the span are not zero"


def test_edge_attention_without_destinations_zeroes_every_edge_row():
    ns = _ops()
    H, C, E = 2, 50, 4
    q, k = torch.randn(0, H * C, device=DEV), torch.randn(E, H * C, device=DEV)
    indptr = torch.zeros(1, dtype=torch.long, device=DEV)
    _nan_fill([(E, H)])
    out, alpha = ns.edge_attn_fwd(q, k, k, k, indptr, H)
    _nan_fill([(E, H * C)])
    dq, dk, dv, de = ns.edge_attn_bwd(q.clone(), q, k, k, k, indptr, alpha, H)
    assert out.shape == (0, H * C) and dq.shape == (0, H * C)
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        print(f"{name} with n_dst = 0: {int(torch.isnan(got).sum())} NaN of {got.numel()}")
    for name, got in (("alpha", alpha), ("dk", dk), ("dv", dv), ("de", de)):
        assert got.size(0) == E and bool((got == 0).all()), f"{name}: n_dst = 0 must leave every edge row zero"


# ------------------------------------------------------------------ col_sum
@pytest.mark.parametrize("M,N", R.COL_SUM_MN)
def test_col_sum_chunk_and_strip_boundaries(M, N):
    ns = _ops()
    x = R.col_sum_case(M, N)
    got = ns.col_sum(x.to(DEV))
    close(got, x.double().sum(0), GRAD_TOL, f"col_sum {M}x{N}")
    assert torch.equal(got, ns.col_sum(x.to(DEV)))


def test_col_sum_row_strided_view_two_chunks():
    ns = _ops()
    wide = R.col_sum_case(257, 172)
    view = wide.to(DEV)[:, 36:101]                                # ldx 172 > N 65, M = 257: two chunks, two strips
    assert not view.is_contiguous()
    got = ns.col_sum(view)
    close(got, wide[:, 36:101].double().sum(0), GRAD_TOL, "col_sum ldx>N")
    assert torch.equal(got, ns.col_sum(view))
    assert torch.equal(got, ns.col_sum(view.contiguous()))       # the order depends on (M, N) alone


# ------------------------------------------------------------------ memory cell
CELL_NAMES = ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh")


@pytest.mark.parametrize("cell", ["gru", "rnn"])
@pytest.mark.parametrize("M,d_in,D", R.CELL_SHAPES)
def test_memory_cell_widths(cell, M, d_in, D):
    from tgnx.ops import memory_cell
    _check(lambda *a: memory_cell(*a, cell), R.cell_case(cell, M, d_in, D), CELL_NAMES,
           f"{cell} M={M} d_in={d_in} D={D}")


def test_memory_cell_width_without_biases():
    from tgnx.ops import memory_cell
    cell, M, d_in, D = R.CELL_NO_BIAS
    _check(lambda *a: memory_cell(*a, cell), R.cell_case(cell, M, d_in, D, False), CELL_NAMES, f"{cell} no bias")


# ------------------------------------------------------------------ link predictor
PRED_NAMES = ("z_src", "z_dst", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out")


@pytest.mark.parametrize("sigmoid", [True, False])
@pytest.mark.parametrize("d_in,D,n_src,k", R.PRED_CASES)
def test_link_predictor_widths(d_in, D, n_src, k, sigmoid):
    from tgnx.ops import link_predictor
    case = R.pred_case(d_in, D, n_src, k, sigmoid)
    out, _ = _check(lambda *a: link_predictor(*a, sigmoid=sigmoid), case, PRED_NAMES,
                    f"pred d_in={d_in} D={D} n_src={n_src} k={k} sig={int(sigmoid)}")
    assert out.shape == (n_src * k, 1)


# ------------------------------------------------------------------ linear, time encoder, time embedding
@pytest.mark.parametrize("M,d_in,d_out,bias", R.LINEAR_CASES)
def test_linear_widths(M, d_in, d_out, bias):
    from tgnx.ops import linear
    _check(linear, R.linear_case(M, d_in, d_out, bias), ("x", "w", "b"), f"linear M={M} {d_in}->{d_out} b={int(bias)}")


def _time_encode_on_gpu(case):
    from tgnx.ops import time_encode
    t, w, b = case["inputs"]

    def run():
        wd, bd = _dev(w, True), _dev(b, True)
        out = time_encode(t.to(DEV), wd, bd)
        out.backward(case["dout"].to(DEV))
        return out, wd.grad, bd.grad
    out, dw, db = run()
    out2, dw2, db2 = run()
    assert torch.equal(out, out2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    return out, dw, db


@pytest.mark.parametrize("n", R.ROW_N)
@pytest.mark.parametrize("D", R.ROW_D)
def test_time_encode_widths(D, n):
    case = R.time_encode_case(n, D)
    out, dw, db = _time_encode_on_gpu(case)
    close(out, case["out"], FWD_TOL, f"time_encode n={n} D={D}")
    close(dw, case["grads"][0], GRAD_TOL, f"time_encode n={n} D={D} dw")
    close(db, case["grads"][1], GRAD_TOL, f"time_encode n={n} D={D} db")


def test_time_encode_arguments_up_to_2_pow_30():
    case = R.time_encode_big_case()
    out, dw, db = _time_encode_on_gpu(case)
    err = float((out.detach().double().cpu() - case["out"]).abs().max())
    print(f"time_encode |w t| <= 2^30: max |out - cos| {err:.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    close(dw, case["grads"][0], GRAD_TOL, "time_encode big dw")
    close(db, case["grads"][1], GRAD_TOL, "time_encode big db")


@pytest.mark.parametrize("n", R.ROW_N)
@pytest.mark.parametrize("D", R.ROW_D)
def test_time_embedding_widths(D, n):
    from tgnx.ops import time_embedding
    case = R.time_embedding_case(n, D)
    out, leaves = _run(time_embedding, case["inputs"], case["dout"])
    close(out, case["out"], FWD_TOL, f"time_embedding n={n} D={D}")
    for name, leaf, want in zip(("x", "w", "b"), (leaves[0], leaves[2], leaves[3]), case["grads"]):
        close(leaf.grad, want, GRAD_TOL, f"time_embedding n={n} D={D} d{name}")
    assert leaves[1].grad is None                                 # rel_t is data
    _, again = _run(time_embedding, case["inputs"], case["dout"])
    for i in (0, 2, 3):
        assert torch.equal(leaves[i].grad, again[i].grad)


# ------------------------------------------------------------------ aggregators
@pytest.mark.parametrize("t_kind", R.AGG_T_KINDS)
@pytest.mark.parametrize("dim", R.AGG_DIMS)
def test_aggregators_at_the_wave_boundary(dim, t_kind):
    from oracle.tgn_ref import last_aggregate, mean_aggregate, scatter_max_first
    from tgnx.ops import aggregate_last, aggregate_mean
    c = R.agg_case(dim, t_kind)
    msg, index, t, dim_size, dout = c["msg"], c["index"], c["t"], c["dim_size"], c["dout"]
    out, arg = _ops().msg_agg_last(msg.to(DEV), index.to(DEV), t.to(DEV), dim_size)
    _, want_arg = scatter_max_first(t, index, dim_size)
    assert torch.equal(arg.cpu(), want_arg)
    for r, want in c["expect_arg"].items():
        assert int(arg[r]) == want, (r, int(arg[r]), want)
    assert torch.equal(out.cpu(), last_aggregate(msg, index, t, dim_size))
    for name, ref_fn, fn in (("last", last_aggregate, lambda m: aggregate_last(m, index.to(DEV), t.to(DEV), dim_size)),
                             ("mean", mean_aggregate, lambda m: aggregate_mean(m, index.to(DEV), dim_size))):
        want32 = ref_fn(msg, index, t, dim_size)
        leaf = msg.detach().double().requires_grad_(True)
        ref_fn(leaf, index, t, dim_size).backward(dout.double())
        grads = []
        for _ in range(2):
            md = _dev(msg, True)
            got = fn(md)
            assert torch.equal(got.detach().cpu(), want32), name    # forward: bit-exact against the fp32 oracle
            got.backward(dout.to(DEV))
            grads.append(md.grad)
        assert torch.equal(grads[0], grads[1])
        if name == "last":                                         # a scatter of dout's rows: exact
            assert torch.equal(grads[0].cpu().double(), leaf.grad), name
        else:
            close(grads[0], leaf.grad, GRAD_TOL, f"mean dmsg dim={dim} t={t_kind}")
