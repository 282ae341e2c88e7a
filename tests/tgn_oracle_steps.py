"""Shared driver of the TGN-against-oracle step comparisons at any ring width, with or without the device's
attention-dropout mask injected into the oracle (test_gpu_tgn_dropout.py, test_gpu_tgn_ring_widths.py).

The comparison is test_gpu_tgn.py's test_tgn_train_steps_and_eval_match_oracle: outputs, loss, every gradient,
memory, last_update and the parameters after Adam per step, the states resynchronised from the oracle after
each step.  Every figure is recorded (and printed) before it is asserted."""
import numpy as np
import torch

import dropout_ref as dr

SHIFT_INVARIANT = {"gnn.conv.lin_key.bias": "gnn.conv.lin_key.weight", "gnn.conv2.lin_key.bias": "gnn.conv2.lin_key.weight"}
ATT_SALT = {"conv": 7, "conv2": 9}       # tgnx_tgn.hip att_salt
CTL_SEED, CTL_NB = 9, 10                 # include/tgnx.h TGNX_CTL_SEED, TGNX_CTL_NB
OUT_TOL, MEM_TOL, GRAD_TOL = 2e-5, 1e-5, 2e-3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@torch.no_grad()
def oracle_embed(ref, lref, ev_t, ev_msg, nodes):
    """The oracle's eval forward for a node set (oracle/tgn_ref.py eval_step, up to the embeddings)."""
    from oracle.tgn_ref import sample_hops
    ref.eval()
    nodes = torch.as_tensor(nodes, dtype=torch.long)
    n_id, ei, e_id = sample_hops(ref, lref, nodes.unique().numpy())
    assoc = torch.zeros(ref.memory.memory.size(0), dtype=torch.long)
    assoc[n_id] = torch.arange(n_id.size(0))
    z, last_update = ref.memory(n_id)
    z = ref.gnn(z, last_update, ei, ev_t[e_id], ev_msg[e_id])
    return z[assoc[nodes]]


class Rig:
    """A RefTGN and a TgnEngine over one synthetic stream, from identical parameters.  The oracle is built with
    dropout 0: its only dropout is the mask a test injects (RefTransformerConv.keep)."""

    def __init__(self, aggr="last", N=300, B=50, d=16, D=32, nb=10, seed=3, ring=10, p=0.0, layers=1, updater="gru",
                 emb=(0, 0), max_neg=20, engine_seed=0, fuse_adam=True):
        from oracle.sampler_ref import RefLastNeighborLoader
        from oracle.tgn_ref import RefTGN
        from tgnx.sampler import LastNeighborLoader
        from tgnx.synth import make_stream
        from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
        self.B, self.p, self.ring, self.N = B, float(p), ring, N
        s = self.s = make_stream("tgbl-wiki", seed=seed, num_events=B * nb, num_nodes=N, msg_dim=d)
        torch.manual_seed(0)
        self.ref = RefTGN(N, d, hidden=D, aggr=aggr, dropout=0.0, layers=layers, updater=updater,
                          use_src_emb_in_msg=bool(emb[0]), use_dst_emb_in_msg=bool(emb[1]))
        self.opt_ref = torch.optim.Adam(self.ref.parameters(), lr=1e-3)
        dev = torch.device("cuda")
        self.model = TGNModel(N, s.num_events, d, D, dev, ring=ring, max_batch=B, max_neg=max_neg, aggr=aggr, dropout=p,
                              layers=layers, updater=updater, memory="dyrep" if updater == "rnn" or any(emb) else "tgn",
                              use_src_emb_in_msg=bool(emb[0]), use_dst_emb_in_msg=bool(emb[1]))
        self.model.load_reference_state(self.ref.state_dict())
        self.opt = TgnAdam(self.model, 1e-3)
        self.eng = TgnEngine(self.model, LastNeighborLoader(N, ring, device=dev),
                             dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg), self.opt,
                             dst_nodes=s.dst_nodes, seed=engine_seed)
        self.eng.fuse_adam = fuse_adam
        self.eng.reset_state()
        self.lref = RefLastNeighborLoader(N, ring)
        self.ev_t = torch.from_numpy(s.t.astype(np.float32))
        self.ev_msg = torch.from_numpy(s.msg)
        self.named = dict(self.ref.named_parameters())
        self.convs = [("conv", self.ref.gnn.conv)] + ([("conv2", self.ref.gnn.conv2)] if layers == 2 else [])
        self.worst = {}

    def batch(self, st):
        sl = slice(st * self.B, (st + 1) * self.B)
        return sl, torch.from_numpy(self.s.src[sl]), torch.from_numpy(self.s.dst[sl])

    def sync(self):
        """Parameters, Adam moments, memory and last_update of the engine from the oracle."""
        model, opt = self.model, self.opt
        with torch.no_grad():
            for name in model.param_order:
                o, n, _ = model._views[name]
                p = self.named[name]
                model.flat[o:o + n].copy_(p.detach().reshape(-1))
                st = self.opt_ref.state.get(p, {})
                if st:
                    opt.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                    opt.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            model.memory.memory.copy_(self.ref.memory.memory)
            model.memory.last_update.copy_(self.ref.memory.last_update)

    def oracle_embed(self, nodes):
        """The oracle's eval-mode embeddings of `nodes` at its current state; changes no state."""
        return oracle_embed(self.ref, self.lref, self.ev_t, self.ev_msg, nodes)

    def _note(self, key, v):
        self.worst[key] = max(self.worst.get(key, 0.0), float(v))

    # ------------------------------------------------------------------ the device's mask, restated
    def sampled(self, src, pos, neg):
        """The oracle's edge list of this batch (before its step inserts the batch): n_id, ei, e_id."""
        from oracle.tgn_ref import sample_hops
        return sample_hops(self.ref, self.lref, torch.cat([src, pos, neg]).unique().numpy())

    def keeps(self, seed, n_id, ei, e_id):
        """{conv name: keep [E, 2]} with values 0 or 1 / (1 - p): key (att_salt, centre node, neighbour e_id), index head."""
        centre = n_id[ei[1]].numpy()
        out = {}
        for name, _ in self.convs:
            base = dr.drop_base(seed, ATT_SALT[name], centre, e_id.numpy())
            out[name] = torch.from_numpy(np.stack([dr.keep_scale(base, h, self.p) for h in (0, 1)], 1).reshape(-1, 2))
        return out

    @torch.no_grad()
    def ref_outputs(self, src, pos, neg):
        """The oracle's training-mode forward of this batch with whatever masks are installed; changes no state."""
        ref = self.ref
        ref.train()
        n_id, ei, e_id = self.sampled(src, pos, neg)
        assoc = torch.zeros(self.N, dtype=torch.long)
        assoc[n_id] = torch.arange(n_id.size(0))
        z, lu = ref.memory(n_id)
        z = ref.gnn(z, lu, ei, self.ev_t[e_id], self.ev_msg[e_id])
        return torch.cat([ref.link_pred(z[assoc[src]], z[assoc[pos]]), ref.link_pred(z[assoc[src]], z[assoc[neg]])]).view(-1)

    # ------------------------------------------------------------------ one compared train step
    def train_step(self, st, neg, dropout=False, out_tol=OUT_TOL, grad_tol=GRAD_TOL, mem_tol=MEM_TOL):
        """Engine step, then the oracle step (with the device's mask if dropout), then the comparison and a resync.
        Returns a dict of what the mask looked like (dropout only): edges, dropped share, keep tensors, n_id, ei,
        and `mask_effect`, the largest change of an oracle output when the mask is removed."""
        from oracle.tgn_ref import train_step
        model, eng, ref = self.model, self.eng, self.ref
        sl, src, pos = self.batch(st)
        pg, ng = eng.train_batch(st * self.B, self.B, neg=neg, dropout=dropout)
        torch.cuda.synchronize()
        eng.check()
        pg, ng = pg.cpu().clone(), ng.cpu().clone()
        info = {}
        if dropout:
            seed, nb = int(eng.ctl[CTL_SEED]), int(eng.ctl[CTL_NB])
            assert seed == dr.step_seed(eng.seed, nb), (st, seed, nb)
            n_id, ei, e_id = self.sampled(src, pos, neg)
            keep = self.keeps(seed, n_id, ei, e_id)
            for _, conv in self.convs:
                conv.keep = None
            plain = self.ref_outputs(src, pos, neg)
            for name, conv in self.convs:
                conv.keep = keep[name]
            masked = self.ref_outputs(src, pos, neg)
            allk = torch.cat([keep[name] for name, _ in self.convs])
            info = dict(edges=int(e_id.numel()), keep=keep, n_id=n_id, ei=ei, e_id=e_id,
                        dropped=float((allk == 0).double().mean()) if allk.numel() else 0.0,
                        mask_effect=float((plain - masked).abs().max()))
        try:
            loss, po, no = train_step(ref, self.opt_ref, self.lref, self.ev_t, self.ev_msg, src, pos, neg,
                                      self.ev_t[sl], self.ev_msg[sl])
        finally:
            for _, conv in self.convs:
                conv.keep = None
        # figures first, asserts after
        fig = {"out": max(float((pg - po).abs().max()), float((ng - no).abs().max())),
               "loss": abs(float(model.grad_flat[-1]) - loss) / max(1.0, abs(loss)),
               "mem": float((model.memory.memory.cpu() - ref.memory.memory).abs().max())}
        g = model.grads_by_name()
        grads = {}
        for name in model.param_order:
            if name in SHIFT_INVARIANT:
                continue
            grads[name] = rel(g[name], self.named[name].grad)
        fig["grad"] = max(grads.values())
        for k, v in fig.items():
            self._note(k, v)
        print(f"step {st}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items())
              + (f" edges={info['edges']} dropped={info['dropped']:.3f} mask_effect={info['mask_effect']:.3e}" if info else ""))
        assert fig["out"] <= out_tol, (st, fig)
        assert fig["loss"] < 1e-5, (st, fig)
        for name in model.param_order:
            if name in SHIFT_INVARIANT:
                scale = float(self.named[SHIFT_INVARIANT[name]].grad.norm()) + 1e-12
                assert float(g[name].norm()) < 1e-4 * scale and float(self.named[name].grad.norm()) < 1e-4 * scale
                continue
            assert grads[name] < grad_tol, (st, name, grads[name])
        assert fig["mem"] <= mem_tol, (st, fig)
        assert torch.equal(model.memory.last_update.cpu(), ref.memory.last_update), st
        for name in model.param_order:
            if name in SHIFT_INVARIANT:
                continue
            o, n, _ = model._views[name]
            assert torch.allclose(model.flat[o:o + n].cpu(), self.named[name].detach().reshape(-1), atol=5e-6, rtol=1e-4), \
                (st, name)
        self.sync()
        return info

    def flush_and_eval(self, st, negs):
        """train(False) on both sides, then one TGB-style eval batch: scores, reciprocal ranks, memory, last_update."""
        from oracle.tgn_ref import eval_step, mrr_per_event
        model, eng, ref = self.model, self.eng, self.ref
        ref.memory.train(False)
        eng.flush()
        torch.cuda.synchronize()
        assert torch.allclose(model.memory.memory.cpu(), ref.memory.memory, atol=MEM_TOL)
        assert torch.equal(model.memory.last_update.cpu(), ref.memory.last_update)
        sl, src, pos = self.batch(st)
        po, no = eval_step(ref, self.lref, self.ev_t, self.ev_msg, src, pos, negs, self.ev_t[sl], self.ev_msg[sl])
        pg, ngm, rr = eng.eval_batch(st * self.B, self.B, negs)
        torch.cuda.synchronize()
        eng.check()
        err = max(float((pg.cpu() - po).abs().max()), float((ngm.cpu() - no).abs().max()))
        self._note("eval_out", err)
        print(f"eval: out={err:.3e}")
        assert err <= OUT_TOL, err
        close = ((no - po.view(-1, 1)).abs() <= 4e-5).any(1).numpy()
        assert np.allclose(rr.cpu().numpy()[~close], mrr_per_event(po, no)[~close], atol=1e-6)
        assert torch.allclose(model.memory.memory.cpu(), ref.memory.memory, atol=MEM_TOL)
        assert torch.equal(model.memory.last_update.cpu(), ref.memory.last_update)
        assert np.array_equal(eng.loader.e_id.cpu().numpy(), self.lref.e_id)
