"""The fused TGNN train step with dropout ON against the oracle's per-block loop, which every other oracle
comparison runs with dropout off (bench.py times the step at the reference's hard-coded 0.6 / 0.6).

The device's three masks are counter-based hashes of (step seed, stream, (block << 32) ^ node-or-root, edge ordinal,
element index); tests/dropout_ref.py restates them and parity_harness.Pair hands them to the oracle
(RefTGNN.drop_keeps), so the oracle computes the same dropped-out step in its own arithmetic: node features and the
residual (stream 1), edge-feature and time-encoding columns (stream 2, the latter at index d + i), attention
(stream 3, index = head).  0.6 / 0.0 and 0.0 / 0.6 make a failure name its stream.

Pair(N 300, E 900, B 150, t_max 5000): a small time scale, so te_w is not chaotic; three steps with a resync from
the oracle between them.  Bounds are test_gpu_tgnn.py's dropout-off ones, unchanged: logits and loss 2e-4 relative
to the batch's largest value, gradients 2e-3 relative to the tensor's largest (attn_r 5e-2, as there), parameters
after Adam 2e-6 where the gradient is above the cancellation floor, ring and time_assoc exact.

So that no case passes vacuously, every step asserts from the restated masks: each active stream's dropped share
lies in [p/2, 2p]; the oracle's logits with and without the masks differ by more than 100x the logit bound; with
attention dropout on, some (block, root, head) with at least two edges loses every edge and some keeps every one."""
import numpy as np
import pytest

from parity_harness import Pair, rel_err

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4


def grad_tol(name):
    return 5e-2 if name.endswith("attn_r") else 2e-3      # test_gpu_tgnn.py: attn_r is a cancellation residue


def _share(masks):
    m = np.concatenate([x.reshape(-1) for x in masks])
    return 1.0 - float(m.mean())


def masks_not_vacuous(p, pf, pa, step):
    """The non-vacuity asserts of one dropout-on step, from the restated masks the oracle was handed (p.masks) and
    p.mask_effect; returns the dropped shares.  Oracle-side only: tests/test_tgnn_widths_cpu.py runs it without a
    GPU."""
    shares = {k: _share(p.masks[k]) for k in ("nfeat", "efeat", "attn")}
    for k, prob in (("nfeat", pf), ("efeat", pf), ("attn", pa)):
        if prob:
            assert prob / 2 <= shares[k] <= 2 * prob, (step, k, shares[k])
        else:
            assert shares[k] == 0.0, (step, k)
    assert p.mask_effect > 100 * LOGIT_TOL, (step, p.mask_effect)
    if pa:
        keep = np.concatenate(p.masks["attn"])                       # [edges, H]
        key = np.concatenate(p.masks["attn_root"])                   # (block << 32) ^ root per edge
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        kept = np.zeros((cnt.size, keep.shape[1]), dtype=np.int64)
        np.add.at(kept, inv, keep.astype(np.int64))
        big = (cnt >= 2)[:, None]
        assert (big & (kept == 0)).any() and (big & (kept == cnt[:, None])).any(), step
    return shares


def dropout_steps_match_oracle(p, pf, pa, steps=3):
    """`steps` dropout-on train steps of Pair `p` against the oracle with the device's masks, a resync between them;
    returns the worst figures.  tests/test_gpu_tgnn_widths.py runs it at other widths."""
    worst = {}
    for step in range(steps):
        if step:
            p.sync_from_ref()
        r = p.train_step(dropout=True)
        fig = {"pos": rel_err(r["pos"], r["ref_pos"]), "neg": rel_err(r["neg"], r["ref_neg"]),
               "loss": abs(r["loss"] - r["ref_loss"]) / max(1.0, abs(r["ref_loss"]))}
        rg, gg = p.ref_grads(), p.gpu_grads()
        grads = {k: rel_err(gg[k], v) for k, v in rg.items()}
        fig["grad"] = max(v for k, v in grads.items() if not k.endswith("attn_r"))
        fig["grad_attn_r"] = max(v for k, v in grads.items() if k.endswith("attn_r"))
        well, allv = p.param_diff()
        fig["param_well"], fig["param_all"] = max(well.values()), max(allv.values())
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
        shares = masks_not_vacuous(p, pf, pa, step)       # the case is not vacuous
        print(f"step {step}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()),
              "dropped:", {k: round(v, 3) for k, v in shares.items()}, f"mask_effect={p.mask_effect:.3e}")
        # the comparison
        assert fig["pos"] < LOGIT_TOL and fig["neg"] < LOGIT_TOL, (step, fig)
        assert fig["loss"] < 2e-4, (step, fig)
        for k, v in grads.items():
            assert v < grad_tol(k), (step, k, v)
        assert fig["param_well"] < 2e-6, (step, well)
        assert fig["param_all"] < 2.5e-4, (step, allv)
        ring_ok, ta_ok = p.state_equal()
        assert ring_ok and ta_ok, step
    print("worst:", {k: f"{v:.3e}" for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("d,pf,pa", [(172, 0.6, 0.6), (1, 0.6, 0.6), (172, 0.6, 0.0), (172, 0.0, 0.6)])
def test_tgnn_dropout_train_steps_match_oracle(d, pf, pa):
    """Measured on an MI355X, worst over the 3 steps and the 4 cases: logits 5.7e-7 (bound 2e-4), loss 1.7e-7
    (2e-4), gradients 4.8e-6 (2e-3), attn_r 8.8e-7 (5e-2), parameters after Adam 3.0e-8 where well conditioned
    (2e-6) and 5.7e-7 overall (2.5e-4).  The dropout-off bounds hold unchanged: no 1 / (1 - p) allowance is taken.
    Removing the masks moves an oracle logit by 0.30 .. 1.06 of the largest (bound: > 2e-2); dropped shares
    0.599 .. 0.606.  With the `d +` offset of the time-encoding mask index removed from the library (forward and
    backward), the three cases with feature dropout fail with logit errors of 0.16 .. 0.26."""
    p = Pair(N=300, E=900, d=d, B=150, Kn_eval=8, seed=3, t_max=5000, feat_drop=pf, attn_drop=pa)
    dropout_steps_match_oracle(p, pf, pa)
