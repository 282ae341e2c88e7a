"""Side-by-side runner: the HIP TGNN step vs the oracle's faithful per-block restatement.

Both start from the same parameters, the same synthetic stream, the same
dependency blocks and the same injected negatives; dropout is off by default (the two
RNG streams cannot be shared).  Used by tests/test_gpu_tgnn.py and by
__graft_entry__.smoke().

Pair(feat_drop=, attn_drop=) + train_step(dropout=True): the HIP step runs with dropout on and the
oracle gets the device's own masks (counter-based hashes, restated in tests/dropout_ref.py) through
RefTGNN.drop_keeps; edge_ordinals() is the map from an oracle edge to the device's mask key.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import blocks_ref
from oracle.epoch_ref import eval_batch as ref_eval_batch
from oracle.epoch_ref import train_batch as ref_train_batch
from oracle.sampler_ref import RefLastNeighborLoader
from oracle.tgnn_ref import RefTGNN

import dropout_ref as dr

CTL_SEED, CTL_NB = 9, 10      # include/tgnx.h TGNX_CTL_SEED, TGNX_CTL_NB


def edge_ordinals(g, sub_e):
    """The ordinal o of each oracle edge of sub_e within its root's segment, as tgnn_meta_collapse's writer
    numbers a segment (tgnx_tgnn.hip edge_meta_body): the root's valid ring slots in slot order, then the self
    loop, then the root's in-batch touches of earlier blocks in touch-key order (block, kind 1 = positive
    destination before kind 2 = source, event).  The oracle's graph lists a node's in-edges in that same order
    by construction: the sampled ring edges row-major over (node, slot) with valid slots leading each row, then
    one self loop per node, then per earlier block the s->p edges (root = positive destination) in event order
    followed by the p->s edges (root = source).  sub_e is ascending and holds every in-edge of its roots, so o
    is the count of earlier edges of sub_e with the same destination."""
    dst = g.dst[sub_e].numpy()
    order = np.argsort(dst, kind="stable")
    d = dst[order]
    first = np.r_[0, np.flatnonzero(d[1:] != d[:-1]) + 1]
    run_start = np.repeat(first, np.diff(np.r_[first, d.size]))
    o = np.empty(d.size, dtype=np.int64)
    o[order] = np.arange(d.size) - run_start
    return o


class Pair:
    def __init__(self, N=400, E=1400, d=172, D=100, K=10, B=200, Kn_eval=20, seed=0, t_max=None, shape=None,
                 feat_drop=0.0, attn_drop=0.0, hub_every=None):
        from tgnx.engine import TgnnEngine
        from tgnx.model import TGNN, getOptimizer
        from tgnx.sampler import LastNeighborLoader
        from tgnx.synth import SHAPES, StreamShape, make_stream

        if shape is None:
            base = SHAPES["tgbl-wiki"]
            shape = StreamShape("parity", N, E, d, True, num_src=int(N * 0.85),
                                t_max=base.t_max if t_max is None else t_max)
            self.s = make_stream(shape, seed=seed)
        else:       # a named TGB shape (full node count), first E events of its stream
            self.s = make_stream(shape, seed=seed, num_events=E)
            N, d = self.s.num_nodes, self.s.shape.msg_dim
        if hub_every:     # a hub: the first event's source is the source of every hub_every-th event, so its
            self.s.src[::hub_every] = self.s.src[0]   # segments gather many in-batch edges of earlier blocks
        self.B, self.K, self.D, self.d, self.N, self.Kn_eval = B, K, D, d, N, Kn_eval
        self.blk = blocks_ref.block_ids(self.s.src, self.s.dst, B)
        self.feats = torch.from_numpy(self.s.msg)
        torch.manual_seed(seed)
        self.pf, self.pa = float(feat_drop), float(attn_drop)
        # the oracle draws no mask of its own: with dropout on it is handed the device's (train_step(dropout=True))
        self.ref = RefTGNN(d, D, N, feat_drop=0.0, attn_drop=0.0)
        self.ref_opt = torch.optim.Adam(self.ref.parameters(), lr=1e-4)
        self.ref_loader = RefLastNeighborLoader(N, K)
        sd = {k: v.detach().clone() for k, v in self.ref.named_parameters()}
        self.model = TGNN(d, D, N, "cuda", ring=K, max_batch=B, max_neg=Kn_eval, feat_drop=feat_drop,
                          attn_drop=attn_drop)
        self.model.load_reference_state(sd)
        self.opt = getOptimizer({"gnn": self.model}, 1e-4)
        self.loader = LastNeighborLoader(N, K, device="cuda")
        self.eng = TgnnEngine(self.model, self.loader, self.feats, self.opt, max_neg=Kn_eval, seed=seed)
        self.rng = np.random.default_rng(seed + 99)
        self.pos = 0

    def _batch(self, B):
        sl = slice(self.pos, self.pos + B)
        self.pos += B
        s = self.s
        t32 = s.t[sl].astype(np.float32)
        return (torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl]), torch.from_numpy(t32),
                torch.from_numpy(s.msg[sl]), torch.from_numpy(self.blk[sl]))

    def prefill(self, n_events, chunk=None):
        """Advance both rings (and the e_id counter) over the next `n_events` events, batch by batch,
        without training: a later step then samples full rings, as mid-epoch (`neighbor_loader.insert`,
        epoch_utils.py:300)."""
        chunk = chunk or self.B
        end = self.pos + n_events
        while self.pos < end:
            n = min(chunk, end - self.pos)
            sl = slice(self.pos, self.pos + n)
            self.pos += n
            t32 = self.s.t[sl].astype(np.float32)
            self.ref_loader.insert(self.s.src[sl], self.s.dst[sl], t32)
            self.loader.insert(torch.from_numpy(self.s.src[sl]), torch.from_numpy(self.s.dst[sl]),
                               torch.from_numpy(t32))

    def device_keeps(self, seed, ring_eid=None):
        """The RefTGNN.drop_keeps callback of one step: the device's masks under the step seed, per block.
        Node features and the residual: stream 1, key (blk << 32) ^ node, sub 0, index = feature dim, p = pf.
        Edge features: stream 2, key (blk << 32) ^ root, sub = the edge's ordinal, index [0, d) the edge-feature
        columns and [d, d + D) the time-encoding columns.  Attention: stream 3, same key and sub, index = head,
        p = pa.  Every mask is recorded in self.masks ({stream: [bool keep arrays]}) with the per-edge roots."""
        d, D, H = self.d, self.D, self.ref.H
        self.masks = {"nfeat": [], "efeat": [], "attn": [], "attn_root": []}

        def keeps(blk, g, sub_e):
            nid = g.nid.numpy()
            root = nid[g.dst[sub_e].numpy()]
            o = edge_ordinals(g, sub_e)
            if ring_eid is not None:     # a ring edge's ordinal is its slot in the root's ring row before the batch
                ring = sub_e.numpy() < ring_eid.shape[0]
                assert np.array_equal(self.ref_loader.e_id[root[ring], o[ring]], ring_eid[sub_e.numpy()[ring]])
            hi = np.int64(blk) << 32
            nb = dr.drop_base(seed, 1, hi ^ nid, 0)
            eb = dr.drop_base(seed, 2, hi ^ root, o)
            ab = dr.drop_base(seed, 3, hi ^ root, o)
            kn = dr.keep_scale(nb[:, None], np.arange(D)[None, :], self.pf)
            ke = dr.keep_scale(eb[:, None], np.arange(d + D)[None, :], self.pf)
            ka = dr.keep_scale(ab[:, None], np.arange(H)[None, :], self.pa)
            touched = np.unique(np.r_[g.src[sub_e].numpy(), g.dst[sub_e].numpy()])   # the rows the block reads
            self.masks["nfeat"].append(kn[touched] != 0)
            self.masks["efeat"].append(ke != 0)
            self.masks["attn"].append(ka != 0)
            self.masks["attn_root"].append(hi ^ root)
            return torch.from_numpy(kn), torch.from_numpy(ke), torch.from_numpy(ka)
        return keeps

    def _train_step_dropout(self, src, dst, t, msg, blk, neg):
        """The HIP step first (its seed is read back and checked against the restated formula), then the oracle
        with the device's masks.  Also records `mask_effect`: the largest change of an oracle logit, relative to
        the largest logit, when the masks are removed."""
        from oracle.epoch_ref import _assemble
        pos, negl, _ = self.eng.train_batch(src, dst, t, msg, blk, neg=neg, dropout=True)
        torch.cuda.synchronize()
        self.eng.check()
        pos, negl = pos.cpu().numpy().copy(), negl.cpu().numpy().copy()
        self.gpu_loss = float(self.model.grad_flat[-1])
        seed, nb = int(self.eng.ctl[CTL_SEED]), int(self.eng.ctl[CTL_NB])
        assert seed == dr.step_seed(self.eng.seed, nb), (seed, nb)
        q = torch.cat([src, dst, neg.reshape(-1)]).unique().numpy()
        ring_eid = self.ref_loader(q)[2]
        self.ref.train()
        with torch.no_grad():       # forward() moves time_assoc: put it back after the two probes
            ta = self.ref.time_assoc.clone()
            outs = []
            for cb in (None, self.device_keeps(seed)):
                self.ref.drop_keeps = cb
                g, bf, bt, blocks = _assemble(self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
                outs.append(torch.cat(self.ref(g, bf, bt, blocks)).view(-1).numpy())
                self.ref.time_assoc.copy_(ta)
        self.mask_effect = rel_err(outs[0], outs[1])
        self.ref.drop_keeps = self.device_keeps(seed, ring_eid)
        try:
            ref = ref_train_batch(self.ref, self.ref_opt, self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
        finally:
            self.ref.drop_keeps = None
        return ref, pos, negl

    def train_step(self, dropout=False):
        src, dst, t, msg, blk = self._batch(self.B)
        neg = torch.from_numpy(self.rng.choice(self.s.dst_nodes, size=src.shape[0]))
        if dropout:
            (ref_loss, ref_pos, ref_neg), pos, negl = self._train_step_dropout(src, dst, t, msg, blk, neg)
            order = np.argsort(blk.numpy(), kind="stable")
            return dict(ref_loss=float(ref_loss), loss=self.gpu_loss, ref_pos=ref_pos.view(-1).numpy(),
                        pos=pos[order], ref_neg=ref_neg.view(-1).numpy(), neg=negl[order])
        ref_loss, ref_pos, ref_neg = ref_train_batch(self.ref, self.ref_opt, self.ref_loader, self.feats, src, dst,
                                                     neg, t, msg, blk)
        pos, negl, _ = self.eng.train_batch(src, dst, t, msg, blk, neg=neg, dropout=False)
        torch.cuda.synchronize()
        self.eng.check()
        order = np.argsort(blk.numpy(), kind="stable")      # reference rows are in block order
        return dict(ref_loss=float(ref_loss), loss=float(self.model.grad_flat[-1]),
                    ref_pos=ref_pos.view(-1).numpy(), pos=pos.cpu().numpy()[order],
                    ref_neg=ref_neg.view(-1).numpy(), neg=negl.cpu().numpy()[order])

    def eval_step(self, quirk=True):
        src, dst, t, msg, blk = self._batch(self.B)
        neg2d = np.stack([self.rng.choice(self.s.dst_nodes, size=self.Kn_eval, replace=False)
                          for _ in range(src.shape[0])])
        neg2d = torch.from_numpy(neg2d.astype(np.int64))
        self.ref.eval()
        ref_mrr, ref_pos, ref_neg = ref_eval_batch(self.ref, self.ref_loader, self.feats, src, dst, neg2d, t, msg,
                                                   blk)
        pos, negl, mrr = self.eng.eval_batch(src, dst, t, msg, blk, neg2d, tile_quirk=quirk)
        torch.cuda.synchronize()
        self.eng.check()
        return dict(ref_mrr=ref_mrr, mrr=float(mrr), ref_pos=ref_pos.numpy(), pos=pos.cpu().numpy(),
                    ref_neg=ref_neg.numpy(), neg=negl.cpu().numpy())

    def sync_from_ref(self):
        """Copy the oracle's parameters and Adam moments into the HIP model, so the next step is
        compared from identical state.  Needed at wiki time scales: cos(w*dt + b) with dt ~ 1e6 makes
        the model chaotic in te_w (1 ulp of w = 1.0 turns the phase by ~0.16 rad), so any two fp32
        implementations drift apart over steps; each step's kernels are still checked exactly."""
        with torch.no_grad():
            for k, p in self.ref.named_parameters():
                if not p.requires_grad:
                    continue
                off, n, _ = self.model._views[k]
                self.model.flat[off:off + n].copy_(p.detach().reshape(-1))
                st = self.ref_opt.state.get(p, {})
                if "exp_avg" in st:
                    self.eng.adam_m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                    self.eng.adam_v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
        self._ill = {}

    def ref_grads(self):
        return {k: p.grad.detach().numpy() for k, p in self.ref.named_parameters() if p.grad is not None}

    def gpu_grads(self):
        return {k: v.detach().cpu().numpy() for k, v in self.model.grads_by_name().items()}

    def param_diff(self, rel_floor=1e-3):
        """Max |param_gpu - param_ref| after the optimizer step, split by gradient conditioning.

        Adam's first steps move a parameter by ~lr * g/|g|, so elements whose gradient is at the
        fp32 cancellation floor (|g| < rel_floor * max|g| of the tensor, e.g. attn_r: er shifts a
        whole softmax) may move by +-lr in either implementation; once ill, an element stays excluded
        (the momentum carries it).  Returns (well, all)."""
        well, allv = {}, {}
        if not hasattr(self, "_ill"):
            self._ill = {}
        for k, p in self.ref.named_parameters():
            if not p.requires_grad or p.grad is None:
                continue
            off, n, shape = self.model._views[k]
            g = self.model.flat[off:off + n].view(shape).cpu().numpy()
            d = np.abs(g - p.detach().numpy())
            gr = np.abs(p.grad.detach().numpy())
            ill = gr <= rel_floor * max(gr.max(), 1e-30)
            self._ill[k] = ill | self._ill.get(k, np.zeros_like(ill))   # Adam momentum carries history
            mask = ~self._ill[k]
            well[k] = float(d[mask].max()) if mask.any() else 0.0
            allv[k] = float(d.max())
        return well, allv

    def state_equal(self):
        eid = self.loader.e_id.cpu().numpy()
        ok = np.array_equal(eid, self.ref_loader.e_id)
        ok &= np.array_equal(self.loader.t.cpu().numpy(), self.ref_loader.t)
        nb = self.loader.neighbors.cpu().numpy()
        ok &= np.array_equal(nb[eid >= 0], self.ref_loader.neighbors[self.ref_loader.e_id >= 0])
        ta_ok = np.array_equal(self.model.time_assoc.cpu().numpy(), self.ref.time_assoc.numpy())
        return bool(ok), bool(ta_ok)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))
