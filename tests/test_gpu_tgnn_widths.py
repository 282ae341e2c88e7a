"""The fused TGNN step (csrc/tgnx_tgnn.hip) against the oracle with a memory table that is not constant, at every
width class the library compiles.

Both `oracle/tgnn_ref._Memory` and `tgnx.model.TGNN` start from the reference's memory table of all ones, and every
other TGNN comparison leaves it there.  The library reads that table by row in four places (the edge's source row in
edge_gather, the root's row in root_er8, the residual in tgnn_pred_train and in the two eval predictors): with a
constant table a kernel that read another node's row, or another column, computes the same bits, and el = U_l .
mem[src] is one constant per head.  Here Pair(memory="randn") gives both sides the same random table, and two probes
of the oracle alone say, at every step, that the step depends on it: `memory_effect` (the table against all ones) and
`source_row_effect` (the table against itself with the rows of the nodes that are not roots of the batch rolled by
one: only ring edges' source rows move) must each change an oracle logit by more than 100x the logit bound.

  1  widths      Pair(N 300, E 900, B 150, 8 eval negatives, t_max 5000 as test_gpu_tgnn_dropout.py, randn memory):
     three train steps with a resync from the oracle between them, then one eval step, at test_gpu_tgnn.py's bounds
     (logits and loss 2e-4, gradients 2e-3 of the tensor's largest and attn_r 5e-2, parameters after Adam 2e-6 where
     well conditioned and 2.5e-4 overall, ring and time_assoc exact, MRR 1e-3).  The edge kernels are templates over
     CF = ceil(d / 64) in 0..5 and CT = 1 + (D > 64); before this file only <1, 2> and <3, 2> had run under a test.
     Each case asserts the instantiation and the lanes of its last column rounds by arithmetic on the table's
     literals, and from the oracle's ring that from the second step on the batch's roots include an empty ring row,
     a partly filled one and a full one.  The seed and the prefill length of each case were chosen on the CPU
     (tests/test_tgnn_widths_cpu.py) so that both probes clear their bound at every step; the first step needs a
     prefilled ring for the source-row probe to see any ring edge at all.
  2  forms       at D = 32, d = 70 (<2, 1>): batch capacity 999 and 1000 with B = 150 (from TGNX_BIG_BATCH = 1000 of
     capacity the step launches tgnn_seg_fwd on its own instead of inside tgnn_pred_train, runs the edge backward
     with 12 waves and the segment backward on GSEG_BIG slabs), and a hub batch whose segments lie on both sides of
     SEG_WIDE = 128 edges.
  3  dropout     test_gpu_tgnn_dropout.py's procedure and non-vacuity asserts at <0, 1> and <2, 2>.
  4  refusals    widths outside check_cfg's domain raise its message and leave a later model clean (the host-only
     half is tests/test_cabi.py::test_tgnn_param_layout_refuses_widths_outside_the_domain).

The clamped loads at the smallest widths, settled on make_ulay / make_lay (no change needed):
  tgnn_pred_train   a wave with n <= 0 rows (from D <= 8, and whenever 3 ceil(D / 4) >= D) loads WsT[d0 D + oc] and
      WdT[d0 D + oc] with d0 <= 3 ceil(D / 4) <= D + 2: at most 3 D floats past the end of WdT, which Ws1, Wd1
      (al4(D) each) and the 320 ones follow inside U, all written or zero; the values are never used (j < n).  At
      D = 1 the indices are 0..3 of an al4(1) = 4 float block.
  root_er8          min(j + 8 k, D - 1) >= 0 for every D >= 1: inside the root's row and U_r's.
  EdgeCols          fidx = min(lane + 64 j, d - 1) exists only for j < CF, and d = 0 selects CF = 0: no feature
      column is formed, the (null) feature pointers of a zero-width table are never dereferenced.
  load_x8           reads DX + 8 e floats: DX is carved at a 256-byte boundary and a row is 32 bytes.
What did need a change: seg_bwd_body skipped a segment whose predictor gradient is exactly zero without writing its
edges' dx, which tgnn_edge_bwd reads for every edge (found by the D = 1 case, see section 1's docstring); at d = 0
the step's null-buffer check refused the zero-width feature table and message batch, whose tensors have no storage;
and the edge backward asks for 156,416 bytes of dynamic LDS at D = 128, d = 192 where its launcher had raised the
limit to 153,600 only.
"""
import numpy as np
import pytest
import torch

from parity_harness import Pair, _segment_sizes, rel_err

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4
EFFECT_MIN = 100 * LOGIT_TOL
COMMON = dict(N=300, E=900, B=150, Kn_eval=8, t_max=5000, memory="randn")
K_SEG_FWD = 6       # include/tgnx.h TGNX_K_SEG_FWD: the kernel probe counts tgnn_seg_fwd's own launches
CTL_ERR = 11        # include/tgnx.h TGNX_CTL_ERR

# (D, d, seed, prefilled events), then what the case's numbers must select: CF, CT, the lanes of the last feature
# column round and of the last time-encoding / memory column round
WIDTHS = [
    ((1, 1, 0, 300), (1, 1, 1, 1)),         # the minimum: kc = 1, three idle predictor waves, nt = 1, H D = 8
    ((3, 0, 0, 300), (0, 1, 0, 3)),         # CF = 0 (time encoding only), odd D, F = D
    ((1, 319, 0, 150), (5, 1, 63, 1)),      # CF = 5, the F = 320 cap at the smallest D
    ((17, 193, 3, 150), (4, 1, 1, 17)),     # nt = 2 with one column in the second tile; CF = 4 with one lane
    ((64, 64, 1, 150), (1, 1, 64, 64)),     # CT = 1 full, second predictor lane round empty, CF = 1 full
    ((65, 65, 0, 300), (2, 2, 1, 1)),       # CT = 2 and the second lane round with one lane; CF = 2 with one lane
    ((64, 256, 0, 150), (4, 1, 64, 64)),    # CF = 4 full at the cap
    ((63, 257, 3, 300), (5, 1, 1, 63)),     # CF = 5 with one lane at the cap, D odd
    ((128, 0, 0, 150), (0, 2, 0, 64)),      # the D cap with no edge features
    ((128, 192, 1, 150), (3, 2, 64, 64)),   # both caps, CF = 3 full: the largest edge backward slab
    ((127, 129, 3, 300), (3, 2, 1, 63)),    # the largest odd D, CF = 3 with one lane
    ((100, 172, 0, 150), (3, 2, 44, 36)),   # the wiki widths: the one instantiation run before, now with varied memory
]
FORM = (32, 70, 2, 150)                     # section 2's widths: <CF 2, CT 1>
HUB = dict(N=300, E=1200, B=300, Kn_eval=8, t_max=5000, memory="randn", D=32, d=70, seed=3, hub_every=2)
HUB_PREFILL = 300
DROPOUT = [(64, 0, 1, 150, 0.6, 0.6), (65, 65, 0, 300, 0.6, 0.6)]      # (D, d, seed, prefilled events, pf, pa)


def grad_tol(name):
    return 5e-2 if name.endswith("attn_r") else 2e-3      # test_gpu_tgnn.py: attn_r is a cancellation residue


def not_vacuous(p, step, effects=True):
    """From the oracle alone: the step saw the memory table, the source rows, and (from the second step) every kind
    of ring row.  p.fills, p.memory_effect and p.source_row_effect are the ones the step just recorded."""
    if effects:
        assert p.memory_effect > EFFECT_MIN, (step, p.memory_effect)
        assert p.source_row_effect > EFFECT_MIN, (step, p.source_row_effect)
    if step >= 1:
        empty, partly, full = p.fills
        assert empty > 0 and partly > 0 and full > 0, (step, p.fills)


def _train_steps_and_eval(p, steps=3, before_step=None):
    """`steps` train steps with a resync between them, a resync and one eval step, with test_gpu_tgnn.py's asserts;
    returns the worst figures."""
    worst = {}

    def note(fig):
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)

    for step in range(steps):
        if step:
            p.sync_from_ref()
        if before_step:
            before_step(p, step)
        r = p.train_step()
        fig = {"pos": rel_err(r["pos"], r["ref_pos"]), "neg": rel_err(r["neg"], r["ref_neg"]),
               "loss": abs(r["loss"] - r["ref_loss"]) / max(1.0, abs(r["ref_loss"]))}
        rg, gg = p.ref_grads(), p.gpu_grads()
        grads = {k: rel_err(gg[k], v) for k, v in rg.items()}
        fig["grad"] = max(v for k, v in grads.items() if not k.endswith("attn_r"))
        fig["grad_attn_r"] = max(v for k, v in grads.items() if k.endswith("attn_r"))
        well, allv = p.param_diff()
        fig["param_well"], fig["param_all"] = max(well.values()), max(allv.values())
        note(fig)
        print(f"step {step}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()),
              f"memory_effect={p.memory_effect:.3e} source_row_effect={p.source_row_effect:.3e} fills={p.fills}")
        if any(v >= grad_tol(k) for k, v in grads.items()):     # name every tensor before the first assert stops
            print("gradients:", {k: f"{v:.3e}" for k, v in grads.items()})
        not_vacuous(p, step)
        assert fig["pos"] < LOGIT_TOL and fig["neg"] < LOGIT_TOL, (step, fig)
        assert fig["loss"] < 2e-4, (step, fig)
        for k, v in grads.items():
            assert v < grad_tol(k), (step, k, v)
        assert fig["param_well"] < 2e-6, (step, well)
        assert fig["param_all"] < 2.5e-4, (step, allv)
        ring_ok, ta_ok = p.state_equal()
        assert ring_ok and ta_ok, step
    return worst, note


def _eval_step(p, worst, note):
    p.sync_from_ref()
    r = p.eval_step(quirk=True)
    fig = {"eval_pos": rel_err(r["pos"], r["ref_pos"]), "eval_neg": rel_err(r["neg"], r["ref_neg"]),
           "mrr": abs(r["mrr"] - r["ref_mrr"])}
    note(fig)
    print("eval: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert fig["eval_pos"] < LOGIT_TOL and fig["eval_neg"] < LOGIT_TOL, fig
    assert fig["mrr"] < 1e-3, fig
    assert all(p.state_equal())
    print("worst:", {k: f"{v:.3e}" for k, v in worst.items()})


# ------------------------------------------------------------------ 1: widths
@pytest.mark.parametrize("case,sel", WIDTHS, ids=[f"D{c[0]}-d{c[1]}" for c, _ in WIDTHS])
def test_tgnn_widths_match_oracle(case, sel):
    """Measured on an MI355X, worst over the 12 cases and their steps: train logits 6.0e-7 and eval logits 3.8e-7
    (bound 2e-4), loss 1.6e-7 (2e-4), gradients 1.5e-4 (2e-3; D = 1, d = 319, where half the tensors are scalars
    — every other case stays at or below 2.9e-6), attn_r 9.6e-7 (5e-2), parameters after Adam 6.0e-8 where well
    conditioned (2e-6) and 2.0e-6 overall (2.5e-4), MRR 1.1e-16 (1e-3).  memory_effect 0.47 .. 1.30 and
    source_row_effect 0.027 .. 0.107 (bound: > 0.02 each).
    Before the fix to seg_bwd_body the D = 1 case failed at its second step with temporal_encoder.w.weight's gradient
    off by 0.21 and parameters by 1.1e-4: a segment whose predictor gradient is exactly zero (every ReLU of the row
    dead, which a one-unit predictor does for about half the events) was skipped without writing its edges' dx, and
    tgnn_edge_bwd then summed what the step before had left there.
    Mutation (a scratch build, not committed): with edge_gather's source row `m.u` replaced by the root's `m.root`,
    tests/test_gpu_tgnn.py passes (8 of 8: the table of ones cannot tell) and all 12 cases here fail at their first
    step with logit errors of 0.032 .. 0.49."""
    D, d, seed, prefill = case
    cf, ct, f_lanes, t_lanes = sel
    assert 1 <= D <= 128 and d >= 0 and d + D <= 320
    assert cf == (d + 63) // 64 and ct == 1 + (D > 64), (D, d)
    assert f_lanes == (d - 64 * (cf - 1) if cf else 0) and t_lanes == D - 64 * (ct - 1), (D, d)
    p = Pair(D=D, d=d, seed=seed, **COMMON)
    p.prefill(prefill)
    worst, note = _train_steps_and_eval(p)
    _eval_step(p, worst, note)


# ------------------------------------------------------------------ 2: forms
@pytest.mark.parametrize("max_batch,big", [(999, False), (1000, True)])
def test_batch_capacity_either_side_of_the_large_batch_forms(max_batch, big):
    """The last small capacity and the first large one, the same B = 150 batches.  What the library exposes of the
    choice is the kernel probe's launch count of tgnn_seg_fwd: one per train step when the segment forward is a
    launch of its own, none when it rides in tgnn_pred_train.  The 12-wave edge backward and the GSEG_BIG segment
    slabs hang on the same `Bmax >= TGNX_BIG_BATCH` and nothing reports them separately; they are compared through
    the gradients.  Measured on an MI355X, either capacity: logits 2.3e-7 (bound 2e-4), gradients 9.4e-7 (2e-3),
    parameters after Adam 4.5e-8 (2.5e-4); memory_effect 0.98 .. 0.99, source_row_effect 0.042 .. 0.060."""
    import ctypes

    from tgnx import _lib
    D, d, seed, prefill = FORM
    assert (d + 63) // 64 == 2 and D <= 64
    p = Pair(D=D, d=d, seed=seed, max_batch=max_batch, **COMMON)
    assert p.model.cfg.max_batch == max_batch and p.B == 150
    p.prefill(prefill)
    _lib.call("tgnx_probe_enable", K_SEG_FWD)
    try:
        worst, note = _train_steps_and_eval(p)
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        _lib.call("tgnx_probe_read", ctypes.byref(ms), ctypes.byref(n))
    finally:
        _lib.call("tgnx_probe_enable", 0)
    assert n.value == (3 if big else 0), (max_batch, n.value)
    _eval_step(p, worst, note)


def test_hub_segments_either_side_of_the_wide_form():
    """A hub that is the source of every second event of B = 300 batches over prefilled rings: its later segments of
    a batch gather more than SEG_WIDE = 128 in-batch edges (lane = edge slot, forward and backward) while every other
    segment stays at or below it.  Two train steps and one eval step.  Measured on an MI355X (largest segment 232 /
    233 / 220 edges in the three batches, 92 .. 105 of 600 segments above 128): train logits 3.0e-7 and eval logits
    2.8e-7 (bound 2e-4), gradients 3.4e-6 (2e-3), parameters after Adam 8.9e-8 (2.5e-4); memory_effect 1.04 .. 1.09,
    source_row_effect 0.067 .. 0.082."""
    p = Pair(**HUB)
    p.prefill(HUB_PREFILL)

    def sizes(p, step):
        s = _segment_sizes(p)
        print(f"step {step}: largest segment {s.max()}, {(s > 128).sum()} above 128 of {s.size}")
        assert (s > 128).any() and (s <= 128).any(), s.max()

    worst, note = _train_steps_and_eval(p, steps=2, before_step=sizes)
    sizes(p, "eval")
    _eval_step(p, worst, note)


# ------------------------------------------------------------------ 3: dropout on
@pytest.mark.parametrize("D,d,seed,prefill,pf,pa", DROPOUT, ids=[f"D{c[0]}-d{c[1]}" for c in DROPOUT])
def test_tgnn_dropout_at_other_widths(D, d, seed, prefill, pf, pa):
    """test_gpu_tgnn_dropout.py's three dropout-on steps, bounds and non-vacuity asserts at <CF 0, CT 1> (no feature
    column: the time-encoding mask index starts at d = 0) and <2, 2> (one lane in each last round, mask indices
    64 and d + 64).  Measured on an MI355X, worst over the 3 steps and the 2 cases: logits 3.2e-7 (bound 2e-4), loss
    8.5e-8 (2e-4), gradients 4.2e-5 (2e-3), attn_r 8.2e-7 (5e-2), parameters after Adam 3.0e-8 where well conditioned
    (2e-6) and 1.5e-6 overall (2.5e-4); removing the masks moves an oracle logit by 0.50 .. 0.90 of the largest,
    dropped shares 0.596 .. 0.601."""
    from test_gpu_tgnn_dropout import dropout_steps_match_oracle
    assert ((d + 63) // 64, 1 + (D > 64)) in ((0, 1), (2, 2))
    p = Pair(D=D, d=d, seed=seed, feat_drop=pf, attn_drop=pa, **COMMON)
    p.prefill(prefill)
    dropout_steps_match_oracle(p, pf, pa)
    assert p.memory_effect > EFFECT_MIN and p.source_row_effect > EFFECT_MIN     # (the last step's, masks off)


# ------------------------------------------------------------------ 4: widths outside the domain
def test_widths_outside_the_domain_are_refused():
    from tgnx.model import TGNN
    bad = [(dict(D=0, d=16), "mem_dim must be in"), (dict(D=129, d=16), "mem_dim must be in"),
           (dict(D=100, d=-1), "msg_dim \\+ mem_dim must be <="), (dict(D=128, d=193), "msg_dim \\+ mem_dim must be <="),
           (dict(D=100, d=16, heads=4), "heads must be 8")]
    for kw, msg in bad:
        with pytest.raises(RuntimeError, match="tgnn: " + msg):
            TGNN(kw["d"], kw["D"], 300, "cuda", num_heads=kw.get("heads", 8), ring=10, max_batch=150, max_neg=8)
    p = Pair(D=3, d=0, seed=0, **COMMON)      # a later valid model: its step ends without an error flag
    p.train_step()
    assert int(p.eng.ctl[CTL_ERR]) == 0
    assert torch.isfinite(p.model.grad_flat).all()
