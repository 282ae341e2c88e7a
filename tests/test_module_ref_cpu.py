"""Are the inputs of the width sweep (test_gpu_module_widths.py) well conditioned?  No GPU needed.

For every shape of the sweep (tests/module_ref.py) the operator is computed twice on the CPU, in float32 and in
float64, from the same float32 inputs, and the float32 result must stay within ONE TENTH of the tolerance the GPU
test uses against the float64 reference (2e-5 forward, 1e-4 gradients; max |a - b| over max(|b|_max, 1)).  If plain
fp32 arithmetic cannot hold a case to a tenth of the tolerance, the input is ill-conditioned and a kernel could fail
the GPU test for the input's reasons rather than its own: the input is changed, never the tolerance.  Each test
prints its table (pytest -s).

The one exception is the forward of the time encoder at arguments up to 2^30: its GPU tolerance is one float ulp at 1
(2^-23), which a float32 result, itself rounded to 2^-24 at 1, cannot beat tenfold.  There the test asserts what the
GPU test relies on instead: numpy's float32 product equals the float64 product rounded once, bit for bit, and
float32 cos of that argument is within 2^-23 of the float64 cos."""
import numpy as np
import pytest
import torch

import module_ref as R

FWD, GRAD = R.FWD_TOL / 10, R.GRAD_TOL / 10


def _row(table, what, a, b, limit):
    err, scale = R.rel_err(a, b)
    table.append((what, err / scale, limit))
    return err / scale


def _report(title, table):
    print(f"\n{title}: fp32 CPU vs float64, max |a - b| / max(|b|_max, 1)")
    worst = {}
    for what, rel, limit in table:
        print(f"  {what:<58s} {rel:.3e}  (limit {limit:g})")
        worst[limit] = max(worst.get(limit, 0.0), rel)
    for limit, rel in sorted(worst.items()):
        print(f"  worst against limit {limit:g}: {rel:.3e}")
    bad = [(w, r, lim) for w, r, lim in table if not r <= lim]
    assert not bad, bad


def _fp32_vs_ref(table, what, fn, case, names):
    out, grads = R.run_ref(fn, case["inputs"], case["dout"], torch.float32)
    _row(table, f"{what} out", out, case["out"], FWD)
    for name, g, want in zip(names, grads, case["grads"]):
        if want is None:
            continue
        assert g is not None and g.shape == want.shape, (what, name)
        _row(table, f"{what} d{name}", g, want, GRAD)


def test_edge_attention_inputs_are_well_conditioned():
    table, peak = [], []
    for H, C in R.ATTN_HC:
        for with_e in (True, False):
            for pattern in R.ATTN_PATTERNS:
                for s in R.ATTN_Q_SCALES:
                    case = R.attn_case(H, C, with_e, pattern, s)
                    what = f"attn H={H} C={C} e={int(with_e)} {pattern} q*{s:g}"
                    fn = R.attn_ref(H)
                    _fp32_vs_ref(table, what, fn, case, ("q", "k", "v", "e"))
                    _row(table, f"{what} alpha", fn.alpha, case["alpha"], FWD)
                    if pattern == "main":
                        q, k, _, e = (None if x is None else x.double() for x in case["inputs"][:4])
                        i =torch.repeat_interleave(torch.arange(q.size(0)), case["deg"])
                        ke = k + (e if e is not None else 0)
                        score = (q[i] * ke).view(-1, H, C).sum(-1) / np.sqrt(C)
                        big = case["deg"][i] > 1                 # a degree-1 destination's alpha is 1 whatever q is
                        peak.append((what, float(score.abs().max()), float(case["alpha"][big].max())))
    _report("edge attention", table)
    print("  largest |score| and largest alpha (destinations with more than one edge) per shape, main degrees:")
    for what, sc, al in peak:
        print(f"  {what:<58s} |score| {sc:8.2f}  alpha {al:.6f}")
    # the q * 8 runs must reach scores expf cannot take without the max subtraction (88.72) somewhere in the sweep
    assert max(sc for what, sc, _ in peak if what.endswith("q*8")) > 88.72


def test_memory_cell_inputs_and_the_plain_formula():
    table = []
    cases = [(c, *s, True) for c in ("gru", "rnn") for s in R.CELL_SHAPES] + [(*R.CELL_NO_BIAS, False)]
    for cell, M, d_in, D, bias in cases:
        case = R.cell_case(cell, M, d_in, D, bias)
        what = f"{cell} M={M} d_in={d_in} D={D} bias={int(bias)}"
        _fp32_vs_ref(table, what, R.cell_ref(cell), case, ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh"))
        # the plain formula is torch's cell: float64 torch.nn.GRUCell / RNNCell from the same tensors
        mod = (torch.nn.GRUCell if cell == "gru" else torch.nn.RNNCell)(d_in, D, bias=bias).double()
        x, h, w_ih, w_hh, b_ih, b_hh = case["inputs"]
        with torch.no_grad():
            mod.weight_ih.copy_(w_ih), mod.weight_hh.copy_(w_hh)
            if bias:
                mod.bias_ih.copy_(b_ih), mod.bias_hh.copy_(b_hh)
        xl, hl = x.double().requires_grad_(True), h.double().requires_grad_(True)
        out = mod(xl, hl)
        out.backward(case["dout"].double())
        got = [out, xl.grad, hl.grad, mod.weight_ih.grad, mod.weight_hh.grad] + \
            ([mod.bias_ih.grad, mod.bias_hh.grad] if bias else [])
        for a, b in zip(got, [case["out"]] + case["grads"]):
            assert R.rel_err(a, b)[0] <= 1e-12, what
    _report("memory cell", table)


def test_link_predictor_inputs_are_well_conditioned():
    table = []
    names = ("z_src", "z_dst", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out")
    for d_in, D, n_src, k in R.PRED_CASES:
        for sigmoid in (True, False):
            case = R.pred_case(d_in, D, n_src, k, sigmoid)
            what = f"pred d_in={d_in} D={D} n_src={n_src} k={k} sig={int(sigmoid)}"
            assert case["margin"] > R.PRED_RELU_MARGIN, (what, case["margin"])
            _fp32_vs_ref(table, what, R.pred_ref(sigmoid), case, names)
    _report("link predictor", table)


def test_linear_time_encoder_time_embedding_inputs_are_well_conditioned():
    table = []
    for M, d_in, d_out, bias in R.LINEAR_CASES:
        _fp32_vs_ref(table, f"linear M={M} {d_in}->{d_out} bias={int(bias)}", R.linear_ref,
                     R.linear_case(M, d_in, d_out, bias), ("x", "w", "b"))
    for D in R.ROW_D:
        for n in R.ROW_N:
            case = R.time_encode_case(n, D)
            out, dw, db = R.time_encode_ref(*case["inputs"], case["dout"], torch.float32)
            _row(table, f"time_encode n={n} D={D} out", out, case["out"], FWD)
            _row(table, f"time_encode n={n} D={D} dw", dw, case["grads"][0], GRAD)
            _row(table, f"time_encode n={n} D={D} db", db, case["grads"][1], GRAD)
            case = R.time_embedding_case(n, D)
            out, grads = R.run_ref(R.time_embedding_ref, case["inputs"], case["dout"], torch.float32)
            _row(table, f"time_embedding n={n} D={D} out", out, case["out"], FWD)
            for name, g, want in zip(("x", "w", "b"), (grads[0], grads[2], grads[3]), case["grads"]):
                _row(table, f"time_embedding n={n} D={D} d{name}", g, want, GRAD)
    _report("linear / time encoder / time embedding", table)


def test_time_encoder_large_arguments_reference():
    case = R.time_encode_big_case()
    t, w, b = case["inputs"]
    arg = case["arg"]
    # numpy's float32 product = the exact (float64) product rounded once = torch's float32 product
    assert torch.equal(arg, (t.double().view(-1, 1) * w.double().view(1, -1)).float())
    assert torch.equal(arg, t.view(-1, 1) * w.view(1, -1))
    assert torch.equal(arg, R.time_arg32(t, w, b))
    assert float(arg.abs().max()) == 2.0 ** 30 and float(arg.min()) < -2.0 ** 28 and float(arg.abs().min()) == 0.0
    err = float((torch.cos(arg).double() - case["out"]).abs().max())
    print(f"\ntime encoder, |w t| up to 2^30: fp32 cos vs float64 cos {err:.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    table = []
    out, dw, db = R.time_encode_ref(t, w, b, case["dout"], torch.float32)
    _row(table, "time_encode big dw", dw, case["grads"][0], GRAD)
    _row(table, "time_encode big db", db, case["grads"][1], GRAD)
    _report("time encoder at large arguments", table)


def test_col_sum_and_mean_aggregator_inputs_are_well_conditioned():
    from oracle.tgn_ref import last_aggregate, mean_aggregate, scatter_max_first
    table = []
    for M, N in R.COL_SUM_MN:
        x = R.col_sum_case(M, N)
        _row(table, f"col_sum {M}x{N}", x.sum(0), x.double().sum(0), GRAD)
    for dim in R.AGG_DIMS:
        for kind in R.AGG_T_KINDS:
            c = R.agg_case(dim, kind)
            _, arg = scatter_max_first(c["t"], c["index"], c["dim_size"])
            for r, want in c["expect_arg"].items():             # the oracle picks what the case was built to pick
                assert int(arg[r]) == want, (dim, kind, r)
            grads = []
            for dt in (torch.float32, torch.float64):
                leaf = c["msg"].detach().to(dt).requires_grad_(True)
                mean_aggregate(leaf, c["index"], c["t"], c["dim_size"]).backward(c["dout"].to(dt))
                grads.append(leaf.grad)
            _row(table, f"mean dmsg dim={dim} t={kind}", grads[0], grads[1], GRAD)
            # last is a copy: exact in every dtype
            assert torch.equal(last_aggregate(c["msg"], c["index"], c["t"], c["dim_size"]).double(),
                               last_aggregate(c["msg"].double(), c["index"], c["t"], c["dim_size"]))
    _report("col_sum / mean aggregator", table)


def test_close_is_the_projects_measure():
    a, b = torch.tensor([1.0, 2.0, 10.0]), torch.tensor([1.0, 2.0, 10.001])
    err, scale = R.rel_err(a, b)
    assert scale == pytest.approx(10.001) and err == pytest.approx(0.001, rel=1e-3)
    R.close(a, b, 1.1e-4)
    with pytest.raises(AssertionError):
        R.close(a, b, 0.9e-4)
    assert R.rel_err(torch.tensor([0.5]), torch.tensor([0.25])) == (0.25, 1.0)     # the scale never drops below 1
    assert R.rel_err(torch.zeros(0), torch.zeros(0)) == (0.0, 1.0)
    with pytest.raises(AssertionError):
        R.close(torch.zeros(2, 1), torch.zeros(2), 1.0)
