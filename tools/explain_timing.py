#!/usr/bin/env python3
"""Timing of TgnEngine.explain at the wiki shape: N = 9,227 nodes, msg_dim 172, D = 100, ring 10, B = 200, after the
first half of the synthetic stream (78,737 events) has been observed in eval mode.  The 200 pairs explained are the
200 events that follow the observed half.

Legs, all in one process, alternating within a window:

  explain          eng.explain(src, dst) end to end (unique, tgnx_tgn_explain, ops.link_loo, the host-side gathers),
                   by="slot"; explain_neighbour: by="neighbour"
  explain_c        the tgnx_tgn_explain call of the same unique nodes alone (through TgnEngine._explain_nodes)
  link_loo         ops.link_loo alone on the z / loo_z / count the explain call produced (four GEMMs + loo_rows)
  score            eng.score of the same pairs (embeds both lists, then the LinkPredictor operator): the yardstick
  embed            eng.embed of the same unique nodes: the launches tgnx_tgn_explain shares, with tgn_embed_gather last
  attention        eng.attention of the same unique nodes (tgnx_tgn_explain without the leave-one-out rows)

and two kernels alone, by the library's kernel probe (the dispatch's own begin / end timestamps):

  tgn_explain_rows_us, loo_rows_us   microseconds per launch over a window of explain calls

A window is `--calls` calls of one leg between two device synchronisations, after one warm-up of every leg; `--windows`
windows per leg.  Prints one JSON line and writes it to --out.

  python tools/explain_timing.py [--windows 3] [--calls 200] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)

K_EXPLAIN, K_LOO_ROWS = 13, 14          # include/tgnx.h TGNX_K_EXPLAIN, TGNX_K_LOO_ROWS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--events", type=int, default=None, help="observe only the first rows of the stream (rehearsal)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "explain.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from tgnx import _lib, ops
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K = args.batch, 100, 10
    N, d = shape.num_nodes, shape.msg_dim
    E = stream.num_events // 2 if args.events is None else min(args.events, stream.num_events - args.pairs)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    events = dict(src=stream.src[:E], dst=stream.dst[:E], t=stream.t[:E].astype(np.float32), msg=stream.msg[:E])
    model = TGNModel(N, E, d, D, dev, ring=K, max_batch=B, max_neg=1, aggr="last", dropout=0.1, generator=gen)
    eng = TgnEngine(model, LastNeighborLoader(N, K, device=dev), events, TgnAdam(model, 1e-4),
                    dst_nodes=np.unique(stream.dst), seed=1234)
    eng.reset_state()
    eng.flush()
    eng.observe_range(0, E, B)
    torch.cuda.synchronize()
    eng.check()
    src = torch.from_numpy(stream.src[E:E + args.pairs].copy()).to(dev)
    dst = torch.from_numpy(stream.dst[E:E + args.pairs].copy()).to(dev)
    uniq = torch.unique(torch.cat([src, dst]))
    first = eng.explain(src, dst)
    w = eng._link_weights()
    z, loo_z, srow, drow = (first[k] for k in ("z", "loo_z", "src_row", "dst_row"))
    count = eng._explain_nodes(uniq, 0, False, True, "timing")["count"]
    legs = {
        "explain": lambda: eng.explain(src, dst),
        "explain_neighbour": lambda: eng.explain(src, dst, by="neighbour"),
        "explain_c": lambda: eng._explain_nodes(uniq, 0, True, False, "timing"),
        "link_loo": lambda: ops.link_loo(z, loo_z, count, srow, drow, *w),
        "score": lambda: eng.score(src, dst),
        "embed": lambda: eng.embed(uniq),
        "attention": lambda: eng.attention(uniq),
    }

    def window(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    def probed(kid, f):
        _lib.call("tgnx_probe_enable", kid)
        for _ in range(args.calls):
            f()
        torch.cuda.synchronize()
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        _lib.call("tgnx_probe_read", ctypes.byref(ms), ctypes.byref(n))
        _lib.call("tgnx_probe_enable", 0)
        return ms.value * 1e3 / max(n.value, 1), int(n.value)

    for f in legs.values():                                        # warm-up of every leg
        f()
    times = {k: [] for k in legs}
    kern = {"tgn_explain_rows_us": [], "loo_rows_us": []}
    for _ in range(args.windows):
        for k, f in legs.items():
            times[k].append(round(window(f), 4))
        kern["tgn_explain_rows_us"].append(round(probed(K_EXPLAIN, legs["explain"])[0], 3))
        kern["loo_rows_us"].append(round(probed(K_LOO_ROWS, legs["explain"])[0], 3))
    eng.check()
    slots = int(count.sum())
    out = {"tool": "explain_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "ring": K,
           "batch": B, "events_observed": E, "pairs": int(src.numel()), "unique_nodes": int(uniq.numel()),
           "valid_slots_of_unique_nodes": slots, "windows": args.windows, "calls_per_window": args.calls,
           "unit": "ms per call, `calls_per_window` calls of one leg between two device synchronisations; *_us: "
                   "microseconds per kernel launch by the kernel probe",
           "ms": times, "kernel_us": kern,
           "median_ms": {k: float(np.median(v)) for k, v in times.items()},
           "median_kernel_us": {k: float(np.median(v)) for k, v in kern.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
