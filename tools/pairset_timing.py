#!/usr/bin/env python3
"""What the live pair history costs and buys at the wiki shape: the synthetic tgbl-wiki stream (N = 9,227 nodes),
mem_dim 100, ring 10, B = 200, half the stream observed by two engines that differ only in enable_pair_history().

  observe      observe() per batch with the history on against off: windows of `--batches` consecutive batches of the
               second half of the stream, the same rows on both engines (one extra launch per batch, and the growth
               rule's host reads where they fall)
  select       PairSet.select for the 200 sources of a batch over all nodes (count, scan, fill and the one host read)
               against the only route without it: PairHistory.build over the whole observed table, contains() on the
               [Q * C] cross product, nonzero — reported with and without the build, and it needs the table kept
  recommend    recommend_filtered(k = 10) for the same sources with exclude_history=True against exclude_seen=True
  rehash       one growth rehash of the observed history into a table of twice the capacity
  forget       forget_nodes of one node with the history on against off (repeat i forgets the i-th busiest node on
               both engines, so the state drifts by one node per repeat)

One call (or one window of batches) between two device synchronisations, after a warm-up of every leg; legs alternate
within a repeat.  Prints one JSON line and writes it to --out.

  python tools/pairset_timing.py [--repeats 7] [--batches 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20, help="batches per observe window")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "pairs.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from tgnx.pairset import PairSet
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgb_negs import PairHistory
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K, R, W = args.batch, 100, 10, args.repeats, args.batches
    N, d = shape.num_nodes, shape.msg_dim
    E = stream.num_events // 2
    rows = min(stream.num_events, E + (R + 1) * W * B)             # the observed half and the timed windows after it
    assert rows >= E + 2 * W * B, "stream too short for the observe windows"
    dev = torch.device("cuda:0")
    events = dict(src=stream.src[:rows], dst=stream.dst[:rows], t=stream.t[:rows].astype(np.float32),
                  msg=stream.msg[:rows])
    dst_nodes = np.unique(stream.dst)

    def build(history):
        gen = torch.Generator().manual_seed(0)
        model = TGNModel(N, rows, d, D, dev, ring=K, max_batch=B, max_neg=1, aggr="last", dropout=0.1, generator=gen)
        eng = TgnEngine(model, LastNeighborLoader(N, K, device=dev), events, TgnAdam(model, 1e-4), dst_nodes=dst_nodes,
                        seed=1234)
        eng.reset_state()
        eng.flush()
        if history:
            eng.enable_pair_history()
        eng.observe_range(0, E, B)
        torch.cuda.synchronize()
        eng.check()
        return eng

    def window(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    on, off = build(True), build(False)
    ps = on._pairs
    info = {"n_keys": ps.n_keys, "capacity": ps.capacity, "growth_reads_over_first_half": ps.reads,
            "batches_over_first_half": -(-E // B)}
    src_q = on.src[E - B:E].clone()
    cand = torch.arange(N, device=dev)
    src_tab, dst_tab = on.src[:E].clone(), on.dst[:E].clone()
    state = ps.state()

    def static_route(build_index=True, idx=None):
        if build_index:
            idx = PairHistory.build(src_tab, dst_tab, N)
        hit = idx.contains(src_q.repeat_interleave(N), cand.repeat(B)).view(B, N)
        return hit.nonzero()

    idx0 = PairHistory.build(src_tab, dst_tab, N)
    grown = []

    def rehash():
        p = grown.pop()
        p.reserve(2 * p.capacity)
        return p

    legs = {
        "select_ms": lambda: ps.select(src_q, cand),
        "static_build_contains_nonzero_ms": lambda: static_route(True),
        "static_contains_nonzero_ms": lambda: static_route(False, idx0),
        "recommend_exclude_history_ms": lambda: on.recommend_filtered(src_q, 10, exclude_history=True),
        "recommend_exclude_seen_ms": lambda: on.recommend_filtered(src_q, 10, exclude_seen=True),
        "rehash_ms": rehash,
    }
    times = {k: [] for k in legs}
    times.update({k: [] for k in ("observe_on_ms_per_batch", "observe_off_ms_per_batch", "forget_on_ms", "forget_off_ms")})

    def fresh():
        p = PairSet(N, ps.capacity, device=dev)
        p.load_state(state)
        grown.append(p)

    def observe(eng, a):
        for b in range(W):
            eng.observe(a + b * B, B)

    busiest = np.argsort(-np.bincount(np.concatenate([stream.src[:E], stream.dst[:E]]), minlength=N))[:R + 1].tolist()
    for rep in range(R + 1):                                       # repeat 0 is the warm-up of every leg
        fresh()
        a = E + rep * W * B
        rec = {}
        for name, f in legs.items():
            rec[name] = window(f)[0]
        for name, eng in (("observe_on_ms_per_batch", on), ("observe_off_ms_per_batch", off)):
            rec[name] = window(lambda: observe(eng, a))[0] / W
        for name, eng in (("forget_on_ms", on), ("forget_off_ms", off)):
            rec[name] = window(lambda: eng.forget_nodes([busiest[rep]]))[0]
        if rep:
            for k, v in rec.items():
                times[k].append(round(v, 4))
    on.check()
    off.check()
    ptr, ids = ps.select(src_q, cand)
    info.update(select_hits=int(ids.numel()), n_keys_end=ps.n_keys, capacity_end=ps.capacity, growth_reads_end=ps.reads,
                rehash_from=int(state["keys"].numel()))
    out = {"tool": "pairset_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "ring": K,
           "batch": B, "events_observed": E, "queries": B, "candidates": N, "batches_per_observe_window": W,
           "unit": "ms per call (observe: ms per batch over a window of consecutive batches), one call or window "
                   "between device synchronisations, legs alternating within a repeat, one warm-up repeat dropped",
           **info, **times, "median": {k: float(np.median(v)) for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
