"""test_gpu_memory_module.py::test_composed_model_trains_like_oracle at the reference's setting, attention dropout
0.1: the reference's getModel composed from tgnx.nn (TGNMemory + GraphAttentionEmbedding(dropout=0.1) + LinkPredictor)
trained under torch.optim.Adam for 4 batches against RefTGN(dropout=0.1) + oracle.tgn_ref.train_step.

Per batch b the seed is the engine's step_seed(20240607, b + 1); the device side calls
gnn(..., seed=seed, dst_key=n_id, edge_key=e_id) and the oracle gets the same mask restated by tests/dropout_ref.py
over (seed, 7, n_id[ei[1]], e_id) in its own edge order (RefTransformerConv.keep), exactly the engine train step's mask
(tests/tgn_oracle_steps.py builds it the same way).  Tolerances, _adam_close and the loop are that test's, unchanged.

So that the mask is not vacuous, every batch that samples edges asserts that removing the mask moves an oracle output
by more than 100 x FWD_TOL; the first batch samples empty rings (nothing to drop yet) and is not judged on that.

MEASURED (MI355X), worst over the 4 batches: loss 8.3e-8, outputs 6.0e-8, gradients 6.2e-7, memory 1.9e-7; batches
1..3 sample 68 / 111 / 134 edges, the mask drops 0.09 / 0.17 / 0.09 of their (edge, head) pairs and moves an oracle
output by 5.0e-2 / 2.2e-2 / 2.9e-2 (bound: > 2e-3).
"""
import numpy as np
import pytest
import torch

import dropout_ref as dr
from attn_dropout_cases import keep_mask
from test_gpu_memory_module import ADAM_EPS, FWD_TOL, GRAD_TOL, LR, _adam_close, _close, _exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BASE_SEED, P = 20240607, 0.1


class _Model(torch.nn.Module):
    """pyg_model_utils.getModel from tgnx.nn, with the reference's attention dropout."""

    def __init__(self, N, d, D):
        super().__init__()
        from tgnx import nn as tnn
        self.memory = tnn.TGNMemory(N, d, D, D, tnn.IdentityMessage(d, D, D), tnn.LastAggregator())
        self.gnn = tnn.GraphAttentionEmbedding(D, D, d, self.memory.time_enc, dropout=P)
        self.link_pred = tnn.LinkPredictor(D)


@torch.no_grad()
def _oracle_outputs(ref, lref, ev_t, ev_msg, src, pos, neg, N):
    """The oracle's training-mode outputs of this batch with whatever mask is installed; changes no state."""
    from oracle.tgn_ref import sample_hops
    ref.train()
    n_id, ei, e_id = sample_hops(ref, lref, torch.cat([src, pos, neg]).unique().numpy())
    assoc = torch.zeros(N, dtype=torch.long)
    assoc[n_id] = torch.arange(n_id.size(0))
    z, lu = ref.memory(n_id)
    z = ref.gnn(z, lu, ei, ev_t[e_id], ev_msg[e_id])
    return torch.cat([ref.link_pred(z[assoc[src]], z[assoc[pos]]), ref.link_pred(z[assoc[src]], z[assoc[neg]])]).view(-1)


def test_composed_model_trains_like_oracle_with_attention_dropout():
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN, sample_hops, train_step
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import make_stream
    N, B, d, D, NB = 300, 50, 16, 32, 4
    s = make_stream("tgbl-wiki", seed=3, num_events=B * NB, num_nodes=N, msg_dim=d)
    assert np.array_equal(s.t, np.floor(s.t)) and float(s.t.max()) < 2 ** 24     # integer times, exact in float32
    torch.manual_seed(0)
    ref = RefTGN(N, d, hidden=D, aggr="last", dropout=P)
    mine = _Model(N, d, D)
    assert mine.gnn.conv.dropout == P and ref.gnn.conv.dropout == P
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
    judged = 0
    for b in range(NB):
        sl = slice(b * B, (b + 1) * B)
        src, pos = torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl])
        neg = torch.from_numpy(rng.choice(s.dst_nodes, size=B))
        seed = dr.step_seed(BASE_SEED, b + 1)
        with torch.no_grad():
            for n, p in mine.named_parameters():
                p.copy_(refs[n].detach().to(DEV))
        # the oracle's mask of this batch, in its own edge order: key (7, centre node, e_id), index head
        n_id_r, ei_r, e_id_r = sample_hops(ref, lref, torch.cat([src, pos, neg]).unique().numpy())
        keep = keep_mask(seed, 7, n_id_r[ei_r[1]].numpy(), e_id_r.numpy(), 2, P)
        if e_id_r.numel() * 2 >= 100:      # the first batch samples empty rings: nothing to drop yet
            ref.gnn.conv.keep = torch.ones_like(keep)
            plain = _oracle_outputs(ref, lref, ev_t, ev_msg, src, pos, neg, N)
            ref.gnn.conv.keep = keep
            masked = _oracle_outputs(ref, lref, ev_t, ev_msg, src, pos, neg, N)
            effect = float((plain - masked).abs().max())
            print(f"batch {b}: {e_id_r.numel()} edges, dropped {float((keep == 0).double().mean()):.3f}, "
                  f"mask effect {effect:.3e}")
            assert effect > 100 * FWD_TOL, (b, effect)
            judged += 1
        ref.gnn.conv.keep = keep
        opt_r = torch.optim.Adam(ref.parameters(), lr=LR, eps=ADAM_EPS)
        opt_m = torch.optim.Adam(mine.parameters(), lr=LR, eps=ADAM_EPS)
        loss_r, po, no = train_step(ref, opt_r, lref, ev_t, ev_msg, src, pos, neg, ev_t[sl], ev_msg[sl])
        ref.gnn.conv.keep = None
        # the same loop on the device
        sg, pg, ng = src.to(DEV), pos.to(DEV), neg.to(DEV)
        opt_m.zero_grad()
        n_id, ei, e_id, _ = lgpu(torch.cat([sg, pg, ng]).unique())
        assoc[n_id] = torch.arange(n_id.numel(), device=DEV)
        z, last_update = mine.memory(n_id)
        z = mine.gnn(z, last_update, ei, ev_t_g[e_id], ev_msg_g[e_id], seed=seed, dst_key=n_id, edge_key=e_id)
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
    assert judged >= 2, judged
