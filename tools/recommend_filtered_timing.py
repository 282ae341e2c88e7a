#!/usr/bin/env python3
"""Timing of filtered and per-source-list top-k recommendation at the wiki shape of tools/recommend_timing.py: N = 9,227
nodes (every node a candidate), D = 100, 200 source nodes, k = 10, the same mid-epoch state.

  a  the unfiltered operator: ops.link_topk(zs, zc, ..., k)
  b  the filtered operator: the sources' neighbour-ring rows (ring 10) as exclusion lists and self-exclusion
  c  the only route to (b)'s answer without it: return_scores=True, a torch mask (built once, outside the timed
     calls) over the [200, 9227] logits, torch.topk
  d  the lists operator with 500 entries per source
  e  the dense filtered operator masked down to the same 500 entries per source (the other 8,727 excluded)
  f  TgnEngine.recommend_filtered(exclude_seen=True) end to end (embed + the ring rows gathered and sorted + top-k)

Windowing as recommend_timing.py: a window is `--iters` calls between two device synchronisations after a warm-up;
`--repeats` windows per leg, the legs alternating inside every repeat, all in one process.  (b) and (c), and (d) and
(e), are checked to return the same ids.  --legs selects legs; --tree runs the package of another checkout (leg a
against the parent commit's library); --parent-json copies such a run's leg a into the output as `a_parent_library`.
Prints one JSON line and writes it to --out.

  python tools/recommend_filtered_timing.py [--iters 20] [--repeats 3] [--legs abcdef] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--negs", type=int, default=999)
    ap.add_argument("--src", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--list-len", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="abcdef")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is loaded")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "recommend_filtered.json"))
    args = ap.parse_args()
    for p in (args.tree, os.path.join(args.tree, "tgb-tgn-dgl_amd")):
        sys.path.insert(0, os.path.abspath(p))
    import numpy as np
    import torch

    from tgnx import ops
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K, Q, k = args.batch, 100, 10, args.src, args.k
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

    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.choice(np.unique(stream.src), Q, replace=False)).to(dev)
    cand = torch.arange(N, device=dev)
    lp = model.link_pred
    w = [t.detach() for t in (lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias,
                              lp.lin_final.weight, lp.lin_final.bias)]
    z = eng.embed(torch.cat([src, cand]))
    zs, zc = z[:Q].contiguous(), z[Q:].contiguous()
    legs = {"a": lambda: ops.link_topk(zs, zc, *w, k)}
    out = {"tool": "recommend_filtered_timing", "dataset": args.dataset, "num_nodes": N, "mem_dim": D, "sources": Q,
           "candidates": N, "k": k, "ring": K, "list_len": args.list_len, "prefill_train_batches": prefill,
           "iters": args.iters, "repeats": args.repeats, "unit": "ms per call"}
    if set(args.legs) - {"a"}:
        eptr, ekey, _ = eng._exclusions(src, True, None)
        seg = torch.arange(Q, device=dev).repeat_interleave(K)
        mask = torch.zeros(Q, N + 1, dtype=torch.bool, device=dev)
        mask[seg, ekey] = True                                   # an invalid ring slot carries the key N
        mask = mask[:, :N].contiguous()
        mask[torch.arange(Q, device=dev), src] = True
        out["excluded_pairs"] = int(mask.sum())

        def leg_c():
            _, _, logits = ops.link_topk(zs, zc, *w, k, return_scores=True)
            v, i = torch.topk(logits.masked_fill(mask, float("-inf")), k, dim=1)
            return torch.sigmoid(v), i

        L = args.list_len
        pos = torch.from_numpy(np.stack([rng.choice(N, L, replace=False) for _ in range(Q)])).to(dev)
        lptr = torch.arange(Q + 1, device=dev) * L
        keep = torch.zeros(Q, N, dtype=torch.bool, device=dev)
        keep[torch.arange(Q, device=dev)[:, None], pos] = True
        comp = (~keep).nonzero()[:, 1].contiguous()              # row-major: each source's excluded positions ascending
        cptr = torch.arange(Q + 1, device=dev) * (N - L)
        legs.update({
            "b": lambda: ops.link_topk(zs, zc, *w, k, cand_key=cand, src_key=src, exclude=(eptr, ekey), validate=False),
            "c": leg_c,
            "d": lambda: ops.link_topk(zs, zc, *w, k, lists=(lptr, pos.view(-1)), validate=False, max_len=L),
            "e": lambda: ops.link_topk(zs, zc, *w, k, exclude=(cptr, comp), validate=False),
            "f": lambda: eng.recommend_filtered(src, k, candidates=cand, exclude_seen=True)})
        # equal logits (nodes without history share one embedding) are ordered by position in b, c and e and by list
        # slot in d: the values agree where the ids of tied candidates may not
        (bv, bi), (cv, ci), (dv, di), (ev, ei) = (legs[n]()[:2] for n in "bcde")
        out["b_vs_c_rows_with_equal_ids"] = int((bi == ci).all(1).sum())
        out["d_vs_e_rows_with_equal_ids"] = int((di == ei).all(1).sum())
        out["d_vs_e_rows_with_equal_values"] = int((dv == ev).all(1).sum())
    names = [n for n in "abcdef" if n in args.legs]
    for n in names:
        restore()
        for _ in range(3):
            legs[n]()                                            # warm-up (allocator, first launches)
        out[n] = []
    for _ in range(args.repeats):
        for n in names:
            restore()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                legs[n]()
            torch.cuda.synchronize()
            out[n].append(round((time.perf_counter() - t0) * 1e3 / args.iters, 4))
    eng.check()
    if args.parent_json:
        with open(args.parent_json) as f:
            out["a_parent_library"] = json.loads(f.readline())["a"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
