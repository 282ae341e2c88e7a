#!/usr/bin/env python3
"""Timing of embedding-space nearest neighbours at the wiki shape of tools/rank_timing.py: N = 9,227 nodes (every node
a candidate), D = 100, 200 query nodes, k = 10, cosine, the query itself excluded, the same mid-epoch state.

  a  the operator alone on a fixed table: ops.embed_knn(table[nodes], table, k, q_key=nodes) (knn_prep, knn_pairs,
     topk_merge: three launches, no [200, 9227] matrix)
  b  the composition a caller writes today on the same operands: F.normalize of both, zq @ zc.T, the self mask
     (scores[rows, nodes] = -inf) and torch.topk
  c  TgnEngine.similar(cached=True) end to end: `c` with a clean table (nothing to re-embed), `c_stale` right after
     one observe(200) (the refresh re-embeds the rows that batch made stale; the observe itself is outside the
     timed span, each call between two device synchronisations)
  d  TgnEngine.similar(cached=False) end to end (embed() of 200 + 9,227 nodes, then the operator)

Windowing as rank_timing.py: a window is a number of calls between two device synchronisations after a warm-up
(--iters-op calls for the two operator legs, whose calls take tens of microseconds, --iters for the engine legs);
`--repeats` windows per leg, the legs alternating inside every repeat, all in one process; the stream state is
restored before every window.  (a) and (b) are checked to select the same nodes.  Every leg reports its windows,
their median and range; `a_median_le_b_median` is the acceptance comparison.  Prints one JSON line and writes it to
--out.

  python tools/similar_timing.py [--iters 20] [--iters-op 2000] [--repeats 5] [--legs abcd] [--commit ID] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--negs", type=int, default=999)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--iters-op", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "similar.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.nn.functional as F

    from tgnx import ops
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K, Q, k = args.batch, 100, 10, args.queries, args.k
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
    eng.enable_embedding_table()

    def restore():
        """The saved stream state and a current table (every row re-embedded, outside the timed windows)."""
        torch.cuda.synchronize()
        for x, y in zip(state, saved):
            x.copy_(y)
        eng.invalidate_embeddings()
        eng.refresh_embeddings()
        torch.cuda.synchronize()

    rng = np.random.default_rng(1)
    nodes = torch.from_numpy(rng.choice(np.unique(np.concatenate([stream.src, stream.dst])), Q, replace=False)).to(dev)
    rows = torch.arange(Q, device=dev)
    table = eng.embedding_table().clone()                       # the fixed operands of (a) and (b)
    zq = table[nodes].contiguous()

    def leg_b():
        s = F.normalize(zq, dim=1) @ F.normalize(table, dim=1).T
        s[rows, nodes] = float("-inf")
        return torch.topk(s, k, dim=1)

    cursor = [0]

    def stale_call():
        """observe(200) outside the timed span, then similar(cached=True); returns the seconds of the latter."""
        cursor[0] += 1
        eng.observe((prefill + cursor[0] - 1) * B, B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.similar(nodes, k, metric=args.metric, cached=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    legs = {
        "a": lambda: ops.embed_knn(zq, table, k, metric=args.metric, q_key=nodes),
        "b": leg_b,
        "c": lambda: eng.similar(nodes, k, metric=args.metric, cached=True),
        "d": lambda: eng.similar(nodes, k, metric=args.metric, cached=False)}
    iters = {"a": args.iters_op, "b": args.iters_op, "c": args.iters, "c_stale": args.iters, "d": args.iters}
    out = {"tool": "similar_timing", "commit": args.commit, "device": torch.cuda.get_device_name(0),
           "dataset": args.dataset, "num_nodes": N, "mem_dim": D, "queries": Q, "candidates": N, "k": k,
           "metric": args.metric, "exclude_self": True, "batch": B, "prefill_train_batches": prefill,
           "iters": iters, "repeats": args.repeats, "unit": "ms per call"}
    assert args.metric == "cosine" or "b" not in args.legs, "leg b is the cosine composition"
    assert (prefill + 3 + args.iters) * B <= eng.num_events, "not enough events after the prefill for leg c_stale"
    got, want = legs["a"](), leg_b()
    out["a_vs_b_rows_with_equal_ids"] = int((got[1] == want[1]).all(dim=1).sum())
    out["a_vs_b_max_value_diff"] = float((got[0] - want[0]).abs().max())
    names = [n for n in ("a", "b", "c", "c_stale", "d") if n[0] in args.legs]
    for n in names:
        restore()
        cursor[0] = 0
        for _ in range(3):
            stale_call() if n == "c_stale" else legs[n]()        # warm-up (allocator, first launches)
        out[n] = {"windows": []}
    for _ in range(args.repeats):
        for n in names:
            restore()
            cursor[0] = 0
            if n == "c_stale":
                ms = sum(stale_call() for _ in range(iters[n])) * 1e3 / iters[n]
            else:
                t0 = time.perf_counter()
                for _ in range(iters[n]):
                    legs[n]()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / iters[n]
            out[n]["windows"].append(round(ms, 4))
    for n in names:
        w = out[n]["windows"]
        out[n].update(median=round(statistics.median(w), 4), min=min(w), max=max(w))
    if "a" in out and "b" in out:
        out["a_median_le_b_median"] = bool(out["a"]["median"] <= out["b"]["median"])
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
