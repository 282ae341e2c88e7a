"""The oracle half of every case of tests/test_gpu_tgnn_widths.py, without a GPU: one train batch per compared step
through RefTGNN alone (a finite loss, finite gradients) and the conditions that keep a case from passing vacuously —
the memory table and the ring edges' source rows each move an oracle logit by more than 100x the logit bound at every
step, the batch's roots include an empty, a partly filled and a full ring row from the second step on, the hub's
segments lie on both sides of 128 edges, and the dropout cases' restated masks drop their share.  The seeds and
prefill lengths in that file's tables were chosen here: a case whose inputs cannot meet its own preconditions fails
on the CPU, before a GPU run."""
import numpy as np
import pytest
import torch

import dropout_ref as dr
from parity_harness import OracleHalf, _segment_sizes
from test_gpu_tgnn_widths import COMMON, DROPOUT, FORM, HUB, HUB_PREFILL, WIDTHS, not_vacuous


def _finite_step(p, step, drop_seed=None):
    loss, pos, neg = p.ref_train_step(drop_seed=drop_seed)
    assert np.isfinite(float(loss)) and torch.isfinite(pos).all() and torch.isfinite(neg).all(), step
    grads = [q.grad for q in p.ref.parameters() if q.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads), step
    assert any(float(g.abs().max()) > 0 for g in grads), step
    not_vacuous(p, step)


@pytest.mark.parametrize("D,d,seed,prefill", [c for c, _ in WIDTHS] + [FORM], ids=lambda v: str(v))
def test_width_cases_meet_their_preconditions(D, d, seed, prefill):
    p = OracleHalf(D=D, d=d, seed=seed, **COMMON)
    assert p.feats.shape == (COMMON["E"], d)
    assert float(p.ref.memory.memory.std()) > 0.5       # the varied table
    p.prefill(prefill)
    for step in range(3):
        _finite_step(p, step)
    assert p.pos + p.B <= p.s.num_events                  # the eval batch is still in the stream


def test_hub_case_meets_its_preconditions():
    p = OracleHalf(**HUB)
    p.prefill(HUB_PREFILL)
    for step in range(2):
        s = _segment_sizes(p)
        assert (s > 128).any() and (s <= 128).any(), (step, s.max())
        _finite_step(p, step)
    s = _segment_sizes(p)                                  # the eval batch
    assert (s > 128).any() and (s <= 128).any() and p.pos + p.B <= p.s.num_events


@pytest.mark.parametrize("D,d,seed,prefill,pf,pa", DROPOUT, ids=lambda v: str(v))
def test_dropout_cases_meet_their_preconditions(D, d, seed, prefill, pf, pa):
    """The device's masks restated under the step seeds the engine will draw (batch counters 1, 2, 3 of base seed
    `seed`), handed to the oracle as the GPU test does."""
    from test_gpu_tgnn_dropout import masks_not_vacuous
    p = OracleHalf(D=D, d=d, seed=seed, feat_drop=pf, attn_drop=pa, **COMMON)
    p.prefill(prefill)
    for step in range(3):
        _finite_step(p, step, drop_seed=dr.step_seed(seed, step + 1))
        masks_not_vacuous(p, pf, pa, step)


def test_default_memory_is_the_reference_table_of_ones():
    p = OracleHalf(N=50, E=60, d=4, D=6, B=20, Kn_eval=2, seed=1)
    assert torch.equal(p.ref.memory.memory, torch.ones(50, 6)) and not p.probes
