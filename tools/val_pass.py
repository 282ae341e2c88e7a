#!/usr/bin/env python3
"""Validation-pass timing of the TGN memory path at the datasets' negative count: a wiki-shaped stream, batches of
200 events, 999 negatives per event, mid-epoch state (half a train epoch replayed, then TGNMemory.train(False)),
as bench.py's val_eval_gpu leg sets it up, over at least 50 validation batches.

  leg a  the per-batch loop pyg_epoch_utils.test() ran before the resident pass: a CPU negatives table sliced per
         batch, TgnEngine.eval_batch, the batch's mean reciprocal rank kept on the device
  leg b  the resident pass: bind_eval_resident + capture_eval once (untimed, as the drop-in pays them once per
         run), then begin_eval + replay_eval_n + eval_mrr

Every repeat of either leg starts from the same restored state, so the two MRRs must be the same float.  Prints one
JSON line.  On a tree without the resident pass (the parent commit) only leg a runs: copy this file there.

The train steps that build the state hold float atomics, so two runs reach slightly different states and MRRs;
--state FILE saves the state of the first run and loads it in the others (parent tree and this one), whose MRRs
are then the same float.

  python tools/val_pass.py [--batches 60] [--repeats 2] [--legs ab] [--group 8] [--state FILE]
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
    ap.add_argument("--negs", type=int, default=999)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--group", type=int, default=8, help="eval steps per captured graph (0 / 1: single steps only)")
    ap.add_argument("--state", default=None, help="file with the mid-epoch state: written if missing, loaded if present "
                                                  "(two trees then evaluate from the same bits: their MRRs must agree)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, eval_negatives, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K = args.batch, 100, 10
    N, d = shape.num_nodes, shape.msg_dim
    nb = min(args.batches, (stream.val_end - stream.train_end) // B)
    assert nb >= 50, f"{nb} validation batches: the stream is too short"
    lo, hi = stream.train_end, stream.train_end + nb * B
    negs = torch.from_numpy(eval_negatives(stream, "val", args.negs, limit=nb * B))
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
    loaded = bool(args.state) and os.path.exists(args.state)
    if loaded:                                         # the mid-epoch state another run (another tree) left
        eng.reset_state()
        with torch.no_grad():
            for x, y in zip(state, torch.load(args.state)):
                x.copy_(y)
    else:
        eng.bind_resident(0, stream.train_end, B, dropout=True)
        eng.begin_epoch()
        eng.capture_resident()
        eng.capture_group(8)
        eng.replay_resident_n(prefill)
        eng.flush()
        torch.cuda.synchronize()
        eng.check()
        if args.state:
            torch.save([x.cpu() for x in state], args.state)
    torch.cuda.synchronize()
    saved = [x.clone() for x in state]

    def restore():
        torch.cuda.synchronize()
        for x, y in zip(state, saved):
            x.copy_(y)
        torch.cuda.synchronize()

    def leg_a():
        perf = []
        for s in range(lo, hi, B):
            _, _, rr = eng.eval_batch(s, B, negs[s - lo:s - lo + B])
            perf.append(rr.clone().mean())
        return float(torch.stack(perf).mean())       # (synchronises)

    def leg_b():
        eng.begin_eval()
        eng.replay_eval_n(nb)
        return eng.eval_mrr()                        # (synchronises)

    out = {"tool": "val_pass", "dataset": args.dataset, "batch": B, "negatives": args.negs, "batches": nb,
           "events": nb * B, "prefill_train_batches": prefill, "group": args.group,
           "state": "loaded" if loaded else "built"}
    legs = []
    if "a" in args.legs:
        legs.append(("eval_batch_loop", leg_a))
    if "b" in args.legs and hasattr(eng, "bind_eval_resident"):
        eng.bind_eval_resident(lo, hi, B, negs)
        eng.capture_eval(group=args.group)
        legs.append(("resident_replay", leg_b))
    for name, fn in legs:
        restore()
        fn()                                         # warm-up pass (allocator, first launches)
        ms, mrrs = [], []
        for _ in range(args.repeats):
            restore()
            t0 = time.perf_counter()
            mrr = fn()
            ms.append((time.perf_counter() - t0) * 1e3 / nb)
            mrrs.append(mrr)
            eng.check()
        assert len(set(mrrs)) == 1, (name, mrrs)
        out[name] = {"ms_per_batch": [round(x, 4) for x in ms], "events_per_s": [round(B / x * 1e3, 1) for x in ms],
                     "mrr": mrrs[0]}
    if len(legs) == 2:
        out["mrr_equal"] = out["eval_batch_loop"]["mrr"] == out["resident_replay"]["mrr"]
        assert out["mrr_equal"], (out["eval_batch_loop"]["mrr"], out["resident_replay"]["mrr"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
