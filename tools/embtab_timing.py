#!/usr/bin/env python3
"""Timing of the embedding table at the wiki shape of tools/rank_timing.py: N = 9,227 nodes (every node a
candidate), D = 100, ring 10, batches of 200, the state after half the train split (resident train steps, then one
flush).  Uncached and cached legs run in one process on one device, alternating inside every repeat; the stream state
is restored before every window and, for the cached legs, the table is made current again (outside the window);
three embed(arange(N)) calls then precede every window, so that no leg starts on a device another leg left idle.

  a  recommend of 200 sources over all nodes, one call bracketed by device synchronisations:
     a_uncached TgnEngine.recommend; a_cached_clean recommend_cached with nothing stale; a_cached_after_observe
     recommend_cached right after one observe(200) (the observe outside the bracket, the refresh of what it staled inside)
  b  tgn_epoch.rank_stream over 50 batches of 200 (rank the batch over all nodes, then observe it), one window per call:
     b_uncached / b_cached, ms per batch; `b_stale_per_batch` is the mean number of rows a batch's refresh recomputed
  c  observe(200) over consecutive batches with the table disabled / enabled (the cost of the touch launch)
  d  a full refresh (invalidate_embeddings, refresh_embeddings) against embed(arange(N))

Prints one JSON line and writes it to --out.

  python tools/embtab_timing.py [--iters 200] [--repeats 5] [--legs abcd] [--commit ID] [--out FILE]
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
    ap.add_argument("--stream-batches", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "embtab.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch

    from tgnx import tgn_epoch
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K, Q, k, NB = args.batch, 100, 10, args.src, args.k, args.stream_batches
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
    # serving from here on: without the train negatives' pool the default candidates are every node in order (the
    # table itself is then the candidate operand); the resident binding keeps the pool alive
    pool, eng.dst_nodes = eng.dst_nodes, None
    model._tgnx_engine, eng._mode_train = eng, False             # (what tgn_epoch.train / test leave: rank_stream finds it)
    e0 = prefill * B
    assert e0 + max(NB, args.iters + 4) * B <= eng.num_events, "not enough events after the prefill"

    allv = torch.arange(N, device=dev)

    def restore(table: bool):
        """The saved stream state; table: enabled and current, else disabled."""
        torch.cuda.synchronize()
        for x, y in zip(state, saved):
            x.copy_(y)
        if table:
            eng.enable_embedding_table()
            eng.invalidate_embeddings()
            eng.refresh_embeddings()
        else:
            eng.disable_embedding_table()
        for _ in range(3):                                       # every window starts behind the same recent device work
            eng.embed(allv)
        torch.cuda.synchronize()

    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.choice(np.unique(stream.src), Q, replace=False)).to(dev)
    cursor = [0]

    def batch_start():
        cursor[0] += 1
        return e0 + (cursor[0] - 1) * B

    def bracketed(call, before=None):
        """ms of one call between two device synchronisations (`before` runs outside the bracket)."""
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def window(call, n):
        """ms per call of n calls between two device synchronisations."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def full_refresh():
        eng.invalidate_embeddings()
        eng.refresh_embeddings()

    it = args.iters
    # name -> (table enabled, ms per call of one measurement)
    legs = {
        "a_uncached": (False, lambda: sum(bracketed(lambda: eng.recommend(src, k)) for _ in range(it)) / it),
        "a_cached_clean": (True, lambda: sum(bracketed(lambda: eng.recommend_cached(src, k)) for _ in range(it)) / it),
        "a_cached_after_observe": (True, lambda: sum(bracketed(lambda: eng.recommend_cached(src, k),
                                                               lambda: eng.observe(batch_start(), B))
                                                     for _ in range(it)) / it),
        "b_uncached": (False, lambda: window(lambda: tgn_epoch.rank_stream(model, ld, e0, e0 + NB * B, B), 1) / NB),
        "b_cached": (True, lambda: window(lambda: tgn_epoch.rank_stream(model, ld, e0, e0 + NB * B, B, cached=True), 1) / NB),
        "c_observe_table_off": (False, lambda: window(lambda: eng.observe(batch_start(), B), it)),
        "c_observe_table_on": (True, lambda: window(lambda: eng.observe(batch_start(), B), it)),
        "d_full_refresh": (True, lambda: window(full_refresh, it)),
        "d_embed_all": (False, lambda: window(lambda: eng.embed(allv), it)),
    }
    out = {"tool": "embtab_timing", "commit": args.commit, "device": torch.cuda.get_device_name(0),
           "dataset": args.dataset, "num_nodes": N, "mem_dim": D, "sources": Q, "candidates": N, "k": k, "ring": K,
           "batch": B, "layers": int(eng.cfg.layers), "prefill_train_batches": prefill, "stream_batches": NB,
           "iters": it, "repeats": args.repeats, "unit": "ms per call (b: ms per batch)"}
    # the stale rows per batch of the prequential pass, and that cached and uncached rank alike (untimed)
    restore(True)
    counts = []
    refresh = eng.refresh_embeddings
    eng.refresh_embeddings = lambda: (lambda ids: (counts.append(int(ids.numel())), ids)[1])(refresh())
    got = tgn_epoch.rank_stream(model, ld, e0, e0 + NB * B, B, cached=True)
    del eng.refresh_embeddings
    restore(False)
    want = tgn_epoch.rank_stream(model, ld, e0, e0 + NB * B, B)
    out["b_stale_per_batch"] = round(float(np.mean(counts[1:])), 1)           # (the first batch's refresh finds nothing)
    out["b_stale_share_of_nodes"] = round(float(np.mean(counts[1:])) / N, 4)
    out["b_mrr_cached"], out["b_mrr_uncached"] = got["mrr"], want["mrr"]
    out["b_ranks_differing"] = int((got["rank"] != want["rank"]).sum())
    names = [n for n in legs if n[0] in args.legs]
    for n in names:
        restore(legs[n][0])
        cursor[0] = 0
        if n[0] != "b":                                          # warm-up (allocator, first launches); b ran above
            it = 3
            legs[n][1]()
            it = args.iters
        out[n] = []
    for _ in range(args.repeats):
        for n in names:
            restore(legs[n][0])
            cursor[0] = 0
            out[n].append(round(legs[n][1](), 4))
    restore(False)
    eng.check()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
