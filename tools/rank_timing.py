#!/usr/bin/env python3
"""Timing of full-catalogue link ranking at the wiki shape of tools/recommend_filtered_timing.py: N = 9,227 nodes (every
node a candidate), D = 100, 200 (source, destination) pairs, the sources' neighbour-ring rows (ring 10) and the
sources themselves excluded, the same mid-epoch state.

  a  the rank operator: ops.link_rank(zs, z[cand + dst], ..., n_count = N, keys, exclusions); `a_op` is
     torch.ops.tgnx.predictor_rank alone, without link_rank's float64 rank (five small torch kernels)
  b  today's route to the same numbers: ops.link_topk(return_scores=True) at k = 1 over the same rows, then a torch
     mask (built once, outside the timed calls), two compares and three sums over the [200, 9227] logits
  c  the filtered top-k operator at k = 10 with the same exclusions (the same pair work plus select and merge)
  d  TgnEngine.rank end to end (embed of 200 + 9,227 + 200 nodes, the ring rows gathered and sorted, the operator);
     `embed` is the embed() call of (d) alone
  e  TgnEngine.rank_events(start, 200) over consecutive batches; `observe` is observe(start, 200) alone over the same

Windowing as recommend_filtered_timing.py: a window is `--iters` calls between two device synchronisations after a
warm-up; `--repeats` windows per leg, the legs alternating inside every repeat, all in one process; the stream state
is restored before every window.  (a) and (b) are checked to give the same counts.  Prints one JSON line and writes
it to --out.

  python tools/rank_timing.py [--iters 20] [--repeats 3] [--legs abcde] [--commit ID] [--out FILE]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "rank.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
        sys.path.insert(0, p)
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
    dst = torch.from_numpy(rng.choice(np.unique(stream.dst), Q, replace=True)).to(dev)
    cand = torch.arange(N, device=dev)
    lp = model.link_pred
    w = [t.detach() for t in (lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias,
                              lp.lin_final.weight, lp.lin_final.bias)]
    nodes = torch.cat([src, cand, dst])
    z = eng.embed(nodes)
    zs, zcd, zc = z[:Q].contiguous(), z[Q:].contiguous(), z[Q:Q + N].contiguous()
    eptr, ekey, _ = eng._exclusions(src, True, None)
    key = torch.cat([cand, dst])
    target = N + torch.arange(Q, device=dev)
    rows = torch.arange(Q, device=dev)
    seg = rows.repeat_interleave(K)
    mask = torch.zeros(Q, N + 1, dtype=torch.bool, device=dev)
    mask[seg, ekey] = True                                       # an invalid ring slot carries the key N
    mask = mask[:, :N].contiguous()
    mask[rows, src] = True
    mask[rows, dst] = True                                       # the target's own node does not compete
    keep = ~mask

    def leg_b():
        logits = ops.link_topk(zs, zcd, *w, 1, sigmoid=False, return_scores=True)[2]
        tl = logits[rows, target]
        L = logits[:, :N]
        ok = keep & ~torch.isnan(L)
        return ((L > tl[:, None]) & ok).sum(1), ((L == tl[:, None]) & ok).sum(1), ok.sum(1), tl

    cursor = [0]

    def batch_start():
        cursor[0] += 1
        return (prefill + cursor[0] - 1) * B

    legs = {
        "a": lambda: ops.link_rank(zs, zcd, *w, target, n_count=N, cand_key=key, src_key=src, exclude=(eptr, ekey),
                                   validate=False),
        "a_op": lambda: ops.load().predictor_rank(zs, zcd, *w, target, N, key, src, eptr, ekey),
        "b": leg_b,
        "c": lambda: ops.link_topk(zs, zc, *w, k, cand_key=cand, src_key=src, exclude=(eptr, ekey), validate=False),
        "d": lambda: eng.rank(src, dst, candidates=cand, exclude_seen=True, exclude_self=True),
        "embed": lambda: eng.embed(nodes),
        "e": lambda: eng.rank_events(batch_start(), B, candidates=cand, exclude_seen=True, exclude_self=True),
        "observe": lambda: eng.observe(batch_start(), B)}
    out = {"tool": "rank_timing", "commit": args.commit, "device": torch.cuda.get_device_name(0),
           "dataset": args.dataset, "num_nodes": N, "mem_dim": D, "sources": Q, "candidates": N, "k": k, "ring": K,
           "batch": B, "prefill_train_batches": prefill, "iters": args.iters, "repeats": args.repeats,
           "unit": "ms per call", "excluded_pairs": int(mask.sum())}
    assert (prefill + 3 + args.iters) * B <= eng.num_events, "not enough events after the prefill for leg e"
    got, want = legs["a"](), leg_b()
    out["a_vs_b_rows_with_equal_counts"] = int(((got[1] == want[0]) & (got[2] == want[1]) & (got[3] == want[2])).sum())
    out["a_vs_b_target_logit_bits_equal"] = bool(torch.equal(got[4].view(torch.int32), want[3].view(torch.int32)))
    out["mean_rank"] = round(float(got[0].mean()), 2)
    extra = {"a_op": "a", "embed": "d", "observe": "e"}
    names = [n for n in ("a", "a_op", "b", "c", "d", "embed", "e", "observe") if extra.get(n, n) in args.legs]
    for n in names:
        restore()
        cursor[0] = 0
        for _ in range(3):
            legs[n]()                                            # warm-up (allocator, first launches)
        out[n] = []
    for _ in range(args.repeats):
        for n in names:
            restore()
            cursor[0] = 0
            t0 = time.perf_counter()
            for _ in range(args.iters):
                legs[n]()
            torch.cuda.synchronize()
            out[n].append(round((time.perf_counter() - t0) * 1e3 / args.iters, 4))
    restore()
    eng.check()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
