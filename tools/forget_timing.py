#!/usr/bin/env python3
"""Timing of TgnEngine.forget_nodes at the wiki shape: N = 9,227 nodes, msg_dim 172, D = 100, ring 10, B = 200, after
the first half of the synthetic stream (78,737 events) has been observed in eval mode.

Two sets are forgotten: the one busiest node of the observed half, and 100 nodes drawn from the nodes seen (seed 0).
Two ways to a state without them, one process, the legs alternating within a repeat:

  forget    forget_nodes on the observed engine: the whole call; split into its plan phase (the id upload,
            tgnx_tgn_forget_plan and the host read of the record) and its apply phase (dropping the bindings,
            tgnx_tgn_forget_apply); and the whole call with compact=True.  Every window starts from the restored
            observed state (table, store, ring, memory, last_update, node_gen, ctl)
  replay    what the code before forget_nodes offered: the history filtered on the host (rows with an endpoint in the
            set dropped), a new model + engine over it (the upload included) and observe_range over all of it;
            `replay_observe_ms` is the observe_range part alone.  It needs the whole history kept, and it also removes
            the nodes' influence on their partners' memory, which forget_nodes does not: the two routes do not end in
            the same memory, only in a state that names none of the nodes

One call per window between two device synchronisations, after one warm-up of every leg; replay is a window of
ceil(E' / B) observe steps.  The counts forget_nodes returns and the rows a compaction keeps are recorded with the times.
Prints one JSON line and writes it to --out.

  python tools/forget_timing.py [--repeats 7] [--out FILE]
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
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--events", type=int, default=None, help="observe only the first rows of the stream (rehearsal)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "forget.json"))
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
    E = stream.num_events // 2 if args.events is None else min(args.events, stream.num_events)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    events = dict(src=stream.src[:E], dst=stream.dst[:E], t=stream.t[:E].astype(np.float32), msg=stream.msg[:E])
    dst_nodes = np.unique(stream.dst)

    def build(ev, rows, params=None):
        model = TGNModel(N, rows, d, D, dev, ring=K, max_batch=B, max_neg=1, aggr="last", dropout=0.1,
                         generator=gen)
        if params is not None:         # (before the flush: it runs the updater over every node with these parameters)
            model.flat.copy_(params)
        eng = TgnEngine(model, LastNeighborLoader(N, K, device=dev), ev, TgnAdam(model, 1e-4), dst_nodes=dst_nodes,
                        seed=1234)
        eng.reset_state()
        eng.flush()
        return eng

    def sync():
        torch.cuda.synchronize()

    eng = build(events, E)
    params = eng.model.flat.clone()
    eng.observe_range(0, E, B)
    sync()
    eng.check()
    m, ld = eng.model, eng.loader
    old_tab, old_store = eng._tab, m.store
    held = [(x, x.clone()) for x in (m.store, ld.neighbors, ld.e_id, ld.t, m.memory.memory, m.memory.last_update,
                                      m.node_gen, eng.ctl)]

    def restore():
        sync()
        if eng._tab is not old_tab:
            eng._install_table(old_tab, E, old_store)
        for x, saved in held:
            x.copy_(saved)
        sync()

    seen, deg = np.unique(np.concatenate([events["src"], events["dst"]]), return_counts=True)
    sets = {"1": [int(seen[np.argmax(deg)])],
            "100": np.random.default_rng(0).choice(seen, size=100, replace=False).tolist()}

    def leg_forget(name):
        ids = sets[name]
        restore()
        t0 = time.perf_counter()
        ws, rec = eng._forget_plan(eng._ids(ids))                  # (ends in the host read of the record)
        t1 = time.perf_counter()
        assert rec[4] == 0
        eng._forget_apply(ws)
        sync()
        t2 = time.perf_counter()
        restore()
        t3 = time.perf_counter()
        counts = eng.forget_nodes(ids)
        sync()
        t4 = time.perf_counter()
        restore()
        t5 = time.perf_counter()
        out = eng.forget_nodes(ids, compact=True)
        sync()
        t6 = time.perf_counter()
        rows = int(out["kept"].numel())
        return {f"forget{name}_plan_ms": (t1 - t0) * 1e3, f"forget{name}_apply_ms": (t2 - t1) * 1e3,
                f"forget{name}_ms": (t4 - t3) * 1e3, f"forget{name}_compact_ms": (t6 - t5) * 1e3}, counts, rows

    def leg_replay(name):
        ids = np.asarray(sets[name])
        sync()
        t0 = time.perf_counter()
        keep = ~(np.isin(events["src"], ids) | np.isin(events["dst"], ids))
        ev = {k: v[keep] for k, v in events.items()}
        n = int(keep.sum())
        t1 = time.perf_counter()
        e2 = build(ev, n, params)
        sync()
        t2 = time.perf_counter()
        e2.observe_range(0, n, B)
        sync()
        t3 = time.perf_counter()
        e2.check()
        return {f"replay{name}_ms": (t3 - t0) * 1e3, f"replay{name}_filter_ms": (t1 - t0) * 1e3,
                f"replay{name}_observe_ms": (t3 - t2) * 1e3}, n, e2

    out = {"tool": "forget_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "ring": K,
           "batch": B, "events_observed": E, "sets": {k: len(v) for k, v in sets.items()},
           "unit": "ms per call, one call per window between device synchronisations (replay: one window of the host "
                   "filter, the engine build and ceil(E' / B) observe steps); legs alternate within a repeat"}
    for name in sets:                                              # warm-up of every leg, and what the routes leave
        _, counts, rows = leg_forget(name)
        _, n, e2 = leg_replay(name)
        rows2 = int(e2.compact_events().numel())
        out[f"set{name}"] = {"counts": counts, "rows_after_forget_compact": rows, "history_rows_kept": n,
                             "rows_after_replay_compact": rows2}
        del e2
    restore()
    out["rows_after_compact_alone"] = int(eng.compact_events().numel())
    legs = {}
    for _ in range(args.repeats):
        for name in sets:
            for f in (leg_forget, leg_replay):
                r = f(name)[0]
                for k, v in r.items():
                    legs.setdefault(k, []).append(round(v, 3))
    out.update(legs)
    out["median"] = {k: float(np.median(v)) for k, v in legs.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
