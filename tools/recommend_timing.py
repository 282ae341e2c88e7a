#!/usr/bin/env python3
"""Timing of read-only TGN inference at the wiki shape: N = 9,227 nodes, D = 100, 200 source nodes, every node a
candidate, k = 10, mid-epoch state (half a train epoch replayed, then TGNMemory.train(False)), as tools/val_pass.py
sets it up.

  embed      TgnEngine.embed of the 200 sources + 9,227 candidates (tgnx_tgn_embed, chunked by the root capacity)
  topk       the fused all-pairs LinkPredictor + top-k alone (ops.link_topk on the embeddings embed returned)
  recommend  TgnEngine.recommend end to end (embed + topk + the position -> node id map)
  tiled      what a caller had before the fused operator, for the top-k alone: torch.ops.tgnx.predictor over the tiled
             n_src x n_cand pairs (a [n_src * n_cand, D] z_dst operand: 738 MB at the full candidate set), then
             torch.topk — with and without building the operand; --tiled-cand sets its candidate count (default: all)

Every timed window is `--iters` calls between two device synchronisations, after a warm-up of the same calls; every
repeat starts from the restored state (the queries change only the generation word).  Prints one JSON line and writes
it to --out.

  python tools/recommend_timing.py [--src 200] [--k 10] [--iters 20] [--repeats 3] [--tiled-cand N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--negs", type=int, default=999, help="the engine's max_neg (the validation pass's): sets the root capacity")
    ap.add_argument("--src", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tiled-cand", type=int, default=0, help="candidates of the tiled leg (0: all nodes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "recommend.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from tgnx import ops
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K = args.batch, 100, 10
    N, d = shape.num_nodes, shape.msg_dim
    dev = torch.device("cuda:0")
    model = TGNModel(N, stream.num_events, d, D, dev, ring=K, max_batch=B, max_neg=args.negs, aggr="last", dropout=0.1,
                     generator=torch.Generator().manual_seed(0))
    eng = TgnEngine(model, LastNeighborLoader(N, K, device=dev),
                    dict(src=stream.src, dst=stream.dst, t=stream.t.astype(np.float32), msg=stream.msg),
                    TgnAdam(model, 1e-4), dst_nodes=np.unique(stream.dst), seed=1234)
    eng.keep_grads = False
    ld = eng.loader
    state = [model.flat, model.memory.memory, model.memory.last_update, model.store, model.node_gen, ld.neighbors,
             ld.e_id, ld.t, eng.ctl]
    prefill = math.ceil(stream.train_end / B) // 2
    eng.bind_resident(0, stream.train_end, B, dropout=True)
    eng.begin_epoch()
    eng.capture_resident()
    eng.capture_group(8)
    eng.replay_resident_n(prefill)
    eng.flush()
    torch.cuda.synchronize()
    eng.check()
    saved = [x.clone() for x in state]

    def restore():
        torch.cuda.synchronize()
        for x, y in zip(state, saved):
            x.copy_(y)
        torch.cuda.synchronize()

    src = torch.from_numpy(np.random.default_rng(1).choice(np.unique(stream.src), args.src, replace=False)).to(dev)
    cand = torch.arange(N, device=dev)
    both = torch.cat([src, cand])
    lp = model.link_pred
    w = [t.detach() for t in (lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias,
                              lp.lin_final.weight, lp.lin_final.bias)]
    z = eng.embed(both)
    zs, zc = z[:args.src].contiguous(), z[args.src:].contiguous()
    nt = args.tiled_cand or N
    zct = zc[:nt].contiguous()
    ns = ops.load()

    def tiled(zd=None):
        # row c * Q + q of z_dst pairs candidate c with source q (the op's `tile` pairing: row i with source i mod Q)
        zd = zct.repeat_interleave(args.src, 0) if zd is None else zd
        s = ns.predictor(zs, zd, *w, False).view(nt, args.src).t()
        return torch.topk(s, min(args.k, nt), dim=1)

    zd_built = zct.repeat_interleave(args.src, 0)
    legs = [("embed", lambda: eng.embed(both)),
            ("topk", lambda: ops.link_topk(zs, zc, *w, args.k)),
            ("recommend", lambda: eng.recommend(src, args.k, candidates=cand)),
            ("tiled_predictor_topk", tiled),
            ("tiled_predictor_topk_operand_prebuilt", lambda: tiled(zd_built))]
    out = {"tool": "recommend_timing", "dataset": args.dataset, "num_nodes": N, "mem_dim": D, "sources": args.src,
           "candidates": N, "k": args.k, "embed_capacity": eng.embed_capacity(), "embed_calls": -(-both.numel() // eng.embed_capacity()),
           "prefill_train_batches": prefill, "iters": args.iters, "tiled_candidates": nt,
           "tiled_operand_mb": round(nt * args.src * D * 4 / 1e6, 1), "unit": "ms per call"}
    for name, fn in legs:
        restore()
        for _ in range(3):
            fn()                                       # warm-up (allocator, first launches)
        ms = []
        for _ in range(args.repeats):
            restore()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.iters)
        eng.check()
        out[name] = [round(x, 4) for x in ms]
    # the two routes rank the same candidates (their logits differ in the last bits: near-ties may swap)
    fv, fi = ops.link_topk(zs, zct, *w, min(args.k, nt), sigmoid=False)
    tv, ti = tiled()
    out["tiled_vs_fused"] = {"rows_with_equal_ids": int((fi == ti).all(1).sum()), "rows": args.src,
                             "max_abs_logit_diff": float((fv - tv).abs().max())}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
