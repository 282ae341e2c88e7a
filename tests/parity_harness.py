"""Side-by-side runner: the HIP TGNN step vs the oracle's faithful per-block restatement.

Both start from the same parameters, the same synthetic stream, the same
dependency blocks and the same injected negatives; dropout is off by default (the two
RNG streams cannot be shared).  Used by tests/test_gpu_tgnn.py and by
__graft_entry__.smoke().

Pair(feat_drop=, attn_drop=) + train_step(dropout=True): the HIP step runs with dropout on and the
oracle gets the device's own masks (counter-based hashes, restated in tests/dropout_ref.py) through
RefTGNN.drop_keeps; edge_ordinals() is the map from an oracle edge to the device's mask key.

OracleHalf is the oracle's side alone (no library: tests/test_tgnn_widths_cpu.py builds it without a GPU); Pair adds
the HIP model, ring and engine.  Pair(memory="randn") replaces the reference's memory table of all ones on both sides
and records memory_effect / source_row_effect at every train step; Pair(max_batch=) sets the model's batch capacity
apart from B; d = 0 gives a zero-width message array.
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


def _segment_sizes(p):
    """In-edge counts of the next batch's source / destination segments, from the oracle's ring and the batch's
    blocks: valid ring entries + the self loop + the root's touches in earlier blocks of the batch."""
    sl = slice(p.pos, p.pos + p.B)
    src, dst, blk = p.s.src[sl], p.s.dst[sl], p.blk[sl]
    valid = (p.ref_loader.e_id >= 0).sum(1)
    sizes = []
    for roots in (src, dst):
        for r, b in zip(roots, blk):
            sizes.append(valid[r] + 1 + int((((src == r) | (dst == r)) & (blk < b)).sum()))
    return np.asarray(sizes)


class OracleHalf:
    """The oracle's side of a Pair, built without the library: the stream, its dependency blocks, RefTGNN with its
    Adam and its ring, the batch cursor and the negatives' generator.

    memory="randn" fills the oracle's memory table with torch.randn(N, D) from a generator seeded with `seed`
    (the reference's own initial state, all ones, otherwise); Pair takes its state dict afterwards, so both sides
    hold the same table.  With a table given, every train step records two probes of the oracle's logits
    (memory_effect, source_row_effect below) that say whether the step could tell a wrong row from the right one."""

    def __init__(self, N=400, E=1400, d=172, D=100, K=10, B=200, Kn_eval=20, seed=0, t_max=None, shape=None,
                 feat_drop=0.0, attn_drop=0.0, hub_every=None, memory=None):
        from tgnx.synth import SHAPES, StreamShape, make_stream

        if shape is None:
            base = SHAPES["tgbl-wiki"]
            shape = StreamShape("parity", N, E, d, True, num_src=int(N * 0.85),
                                t_max=base.t_max if t_max is None else t_max)
            self.s = make_stream(shape, seed=seed)
        else:       # a named TGB shape (full node count), first E events of its stream
            self.s = make_stream(shape, seed=seed, num_events=E)
            N, d = self.s.num_nodes, self.s.shape.msg_dim
        if self.s.msg.shape != (self.s.num_events, d):      # (d = 0: a zero-width message array)
            self.s.msg = np.zeros((self.s.num_events, d), dtype=np.float32)
        if hub_every:     # a hub: the first event's source is the source of every hub_every-th event, so its
            self.s.src[::hub_every] = self.s.src[0]   # segments gather many in-batch edges of earlier blocks
        self.B, self.K, self.D, self.d, self.N, self.Kn_eval = B, K, D, d, N, Kn_eval
        self.blk = blocks_ref.block_ids(self.s.src, self.s.dst, B)
        self.feats = torch.from_numpy(self.s.msg)
        torch.manual_seed(seed)
        self.pf, self.pa = float(feat_drop), float(attn_drop)
        # the oracle draws no mask of its own: with dropout on it is handed the device's (train_step(dropout=True))
        self.ref = RefTGNN(d, D, N, feat_drop=0.0, attn_drop=0.0)
        assert memory in (None, "randn"), memory
        self.probes = memory is not None
        if memory == "randn":
            with torch.no_grad():
                self.ref.memory.memory.copy_(torch.randn(N, D, generator=torch.Generator().manual_seed(seed)))
        self.ref_opt = torch.optim.Adam(self.ref.parameters(), lr=1e-4)
        self.ref_loader = RefLastNeighborLoader(N, K)
        self.seed = int(seed)
        self.rng = np.random.default_rng(seed + 99)
        self.pos = 0

    def _batch(self, B):
        sl = slice(self.pos, self.pos + B)
        self.pos += B
        s = self.s
        t32 = s.t[sl].astype(np.float32)
        return (torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl]), torch.from_numpy(t32),
                torch.from_numpy(s.msg[sl]), torch.from_numpy(self.blk[sl]))

    def _draw_train(self):
        """The next train batch and its injected negatives (one per event)."""
        src, dst, t, msg, blk = self._batch(self.B)
        neg = torch.from_numpy(self.rng.choice(self.s.dst_nodes, size=src.shape[0]))
        return src, dst, t, msg, blk, neg

    def _prefill_ref(self, sl):
        self.ref_loader.insert(self.s.src[sl], self.s.dst[sl], self.s.t[sl].astype(np.float32))

    def prefill(self, n_events, chunk=None):
        """Advance the ring (and the e_id counter) over the next `n_events` events, batch by batch,
        without training: a later step then samples full rings, as mid-epoch (`neighbor_loader.insert`,
        epoch_utils.py:300)."""
        chunk = chunk or self.B
        end = self.pos + n_events
        while self.pos < end:
            n = min(chunk, end - self.pos)
            sl = slice(self.pos, self.pos + n)
            self.pos += n
            self._prefill_ref(sl)

    def root_fills(self, batch):
        """How many of the batch's roots (sources, destinations and negatives, each once) have an empty, a partly
        filled and a full ring row before the batch."""
        src, dst, _, _, _, neg = batch
        roots = torch.cat([src, dst, neg.reshape(-1)]).unique().numpy()
        n = np.bincount((self.ref_loader.e_id[roots] >= 0).sum(1), minlength=self.K + 1)
        return int(n[0]), int(n[1:self.K].sum()), int(n[self.K])

    def _logits_with_memory(self, table, batch):
        """The oracle's logits of `batch` with `table` in place of its memory (no_grad; time_assoc, which forward()
        moves, and the table are put back)."""
        from oracle.epoch_ref import _assemble
        src, dst, t, msg, blk, neg = batch
        mem = self.ref.memory.memory
        with torch.no_grad():
            ta, keep = self.ref.time_assoc.clone(), mem.detach().clone()
            mem.copy_(table)
            g, bf, bt, blocks = _assemble(self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
            out = torch.cat(self.ref(g, bf, bt, blocks)).view(-1).numpy().copy()
            mem.copy_(keep)
            self.ref.time_assoc.copy_(ta)
        return out

    def probe_memory(self, batch):
        """Two probes of the oracle alone (masks off), each the rel_err of its logits between two tables:
        memory_effect       the case's table against all ones: what a constant table hides;
        source_row_effect   the case's table against itself with the rows of every node that is not a root of the
                            batch rolled by one among themselves.  Roots' rows (er, the residual, the in-batch
                            edges' sources) stay, so only el = U_l . mem[src] of ring edges whose source is not a
                            root moves: what a kernel that gathered another node's row would change."""
        src, dst, _, _, _, neg = batch
        table = self.ref.memory.memory.detach().clone()
        base = self._logits_with_memory(table, batch)
        self.memory_effect = rel_err(self._logits_with_memory(torch.ones_like(table), batch), base)
        roots = torch.cat([src, dst, neg.reshape(-1)]).unique().numpy()
        other = np.setdiff1d(np.arange(self.N), roots)
        rolled = table.clone()
        rolled[other] = table[np.roll(other, 1)]
        self.source_row_effect = rel_err(self._logits_with_memory(rolled, batch), base)
        return self.memory_effect, self.source_row_effect

    def ref_train_step(self, batch=None, drop_seed=None):
        """One train batch through the oracle alone (what Pair.train_step runs beside the HIP step).  drop_seed: the
        step seed whose restated device masks (device_keeps) the oracle is handed."""
        from oracle.epoch_ref import _assemble
        batch = batch or self._draw_train()
        src, dst, t, msg, blk, neg = batch
        self.fills = self.root_fills(batch)
        if self.probes:
            self.probe_memory(batch)
        if drop_seed is None:
            return ref_train_batch(self.ref, self.ref_opt, self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
        q = torch.cat([src, dst, neg.reshape(-1)]).unique().numpy()
        ring_eid = self.ref_loader(q)[2]
        self.ref.train()
        with torch.no_grad():       # forward() moves time_assoc: put it back after the two probes
            ta = self.ref.time_assoc.clone()
            outs = []
            for cb in (None, self.device_keeps(drop_seed)):
                self.ref.drop_keeps = cb
                g, bf, bt, blocks = _assemble(self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
                outs.append(torch.cat(self.ref(g, bf, bt, blocks)).view(-1).numpy())
                self.ref.time_assoc.copy_(ta)
        self.mask_effect = rel_err(outs[0], outs[1])
        self.ref.drop_keeps = self.device_keeps(drop_seed, ring_eid)
        try:
            return ref_train_batch(self.ref, self.ref_opt, self.ref_loader, self.feats, src, dst, neg, t, msg, blk)
        finally:
            self.ref.drop_keeps = None

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


class Pair(OracleHalf):
    """OracleHalf + the HIP model, loader and engine started from the oracle's state dict (memory table included).
    max_batch: the model's batch capacity where it is to differ from B (the library picks its large-batch forms by
    capacity)."""

    def __init__(self, N=400, E=1400, d=172, D=100, K=10, B=200, Kn_eval=20, seed=0, t_max=None, shape=None,
                 feat_drop=0.0, attn_drop=0.0, hub_every=None, memory=None, max_batch=None):
        from tgnx.engine import TgnnEngine
        from tgnx.model import TGNN, getOptimizer
        from tgnx.sampler import LastNeighborLoader

        super().__init__(N=N, E=E, d=d, D=D, K=K, B=B, Kn_eval=Kn_eval, seed=seed, t_max=t_max, shape=shape,
                         feat_drop=feat_drop, attn_drop=attn_drop, hub_every=hub_every, memory=memory)
        N, d = self.N, self.d
        sd = {k: v.detach().clone() for k, v in self.ref.named_parameters()}
        self.model = TGNN(d, D, N, "cuda", ring=K, max_batch=B if max_batch is None else max_batch, max_neg=Kn_eval,
                          feat_drop=feat_drop, attn_drop=attn_drop)
        self.model.load_reference_state(sd)
        self.opt = getOptimizer({"gnn": self.model}, 1e-4)
        self.loader = LastNeighborLoader(N, K, device="cuda")
        self.eng = TgnnEngine(self.model, self.loader, self.feats, self.opt, max_neg=Kn_eval, seed=seed)

    def _prefill_ref(self, sl):
        super()._prefill_ref(sl)
        self.loader.insert(torch.from_numpy(self.s.src[sl]), torch.from_numpy(self.s.dst[sl]),
                           torch.from_numpy(self.s.t[sl].astype(np.float32)))

    def _train_step_dropout(self, batch):
        """The HIP step first (its seed is read back and checked against the restated formula), then the oracle
        with the device's masks.  Also records `mask_effect`: the largest change of an oracle logit, relative to
        the largest logit, when the masks are removed."""
        src, dst, t, msg, blk, neg = batch
        pos, negl, _ = self.eng.train_batch(src, dst, t, msg, blk, neg=neg, dropout=True)
        torch.cuda.synchronize()
        self.eng.check()
        pos, negl = pos.cpu().numpy().copy(), negl.cpu().numpy().copy()
        self.gpu_loss = float(self.model.grad_flat[-1])
        seed, nb = int(self.eng.ctl[CTL_SEED]), int(self.eng.ctl[CTL_NB])
        assert seed == dr.step_seed(self.eng.seed, nb), (seed, nb)
        return self.ref_train_step(batch, drop_seed=seed), pos, negl

    def train_step(self, dropout=False):
        batch = self._draw_train()
        src, dst, t, msg, blk, neg = batch
        if dropout:
            (ref_loss, ref_pos, ref_neg), pos, negl = self._train_step_dropout(batch)
            order = np.argsort(blk.numpy(), kind="stable")
            return dict(ref_loss=float(ref_loss), loss=self.gpu_loss, ref_pos=ref_pos.view(-1).numpy(),
                        pos=pos[order], ref_neg=ref_neg.view(-1).numpy(), neg=negl[order])
        ref_loss, ref_pos, ref_neg = self.ref_train_step(batch)
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
