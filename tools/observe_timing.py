#!/usr/bin/env python3
"""Timing of score-free stream ingestion at the wiki shape: N = 9,227 nodes, msg_dim 172, D = 100, B = 200, mid-epoch
state (half a train epoch replayed, then TGNMemory.train(False)), as tools/recommend_timing.py sets it up.

Three ways to advance memory, message stores and ring over the next `--iters` batches of the stream, one process:

  observe        TgnEngine.observe per batch (tgnx_tgn_observe_step: no negatives, no forward, no score)
  eval_kn1       TgnEngine.eval_batch with 1 negative per event — the cheapest way to advance state without observe
  eval_kn999     TgnEngine.eval_batch with 999 negatives per event (a TGB validation batch)

Every call includes its batch-descriptor launch (tgnx_tgnn_advance), as the engine methods issue it.  Every timed window
is `--iters` consecutive batches between two device synchronisations, after a warm-up of the same calls; every repeat
starts from the restored state.  The three legs leave the same memory / stores / ring (checked once, bit for bit).
Prints one JSON line and writes it to --out.

  python tools/observe_timing.py [--iters 400] [--repeats 5] [--legs observe,eval_kn1,eval_kn999] [--out FILE]
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
    ap.add_argument("--negs", type=int, default=999, help="negatives of the large eval leg (and the engine's max_neg)")
    ap.add_argument("--iters", type=int, default=400, help="consecutive batches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="observe,eval_kn1,eval_kn999")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "observe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

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

    first = prefill * B
    iters = min(args.iters, (stream.num_events - first) // B)
    dst_nodes = np.unique(stream.dst)
    rng = np.random.default_rng(2)
    negs = {kn: torch.from_numpy(rng.choice(dst_nodes, size=(iters * B, kn))).to(dev) for kn in (1, args.negs)}

    def run(leg):
        for i in range(iters):
            a = first + i * B
            if leg == "observe":
                eng.observe(a, B)
            else:
                kn = 1 if leg == "eval_kn1" else args.negs
                eng.eval_batch(a, B, negs[kn][i * B:(i + 1) * B])

    out = {"tool": "observe_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "batch": B,
           "negs": args.negs, "prefill_train_batches": prefill, "first_row": first, "iters": iters,
           "unit": "ms per batch (one advance + one step), windows of `iters` batches between device synchronisations"}
    ends = {}
    legs = [x for x in args.legs.split(",") if x]
    for leg in legs:
        if leg not in ("observe", "eval_kn1", "eval_kn999"):
            raise SystemExit(f"unknown leg {leg!r}")
        restore()
        run(leg)                                           # warm-up (allocator, first launches)
        out[leg] = []
    for _ in range(args.repeats):                          # the legs alternate within a repeat
        for leg in legs:
            restore()
            t0 = time.perf_counter()
            run(leg)
            torch.cuda.synchronize()
            out[leg].append(round((time.perf_counter() - t0) * 1e3 / iters, 4))
            eng.check()
            ends[leg] = [x.clone() for x in state[1:8]]
    if "observe" in ends:    # memory, last_update, stores, node_gen, ring: the eval legs leave what observe leaves
        out["state_equal_to_observe"] = {leg: all(torch.equal(x, y) for x, y in zip(ends[leg], ends["observe"]))
                                         for leg in ends if leg != "observe"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
