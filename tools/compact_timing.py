#!/usr/bin/env python3
"""Timing of event-table compaction and the stream-state checkpoint at the wiki shape: N = 9,227 nodes, msg_dim 172,
D = 100, ring 10, B = 200, after the WHOLE synthetic stream (157,474 events) has been observed in eval mode.

Three ways to a small fresh stream state, one process, the legs alternating within a repeat:

  compact   TgnEngine.compact_events on the observed engine, split into its plan phase (tgnx_tgn_compact_plan and the
            host read of the record) and its apply phase (allocations, tgnx_tgn_compact_apply, the swap); every repeat
            starts from the restored uncompacted table, store, ring and ctl
  replay    what the code before compaction offered: a new model + engine over the full history (the upload of the
            table included) and observe_range over all of it; `replay_observe_ms` is the observe_range part alone
  load      a new model + engine over a one-row table and load_stream_state of the compacted state read back from a
            torch.save file (`load_ms` is load_stream_state alone, host-to-device copies included)

compact and load are one call per window — the call is the unit of work a server issues — between two device
synchronisations, after one warm-up call of every leg; replay is a window of ceil(E / B) observe steps.  Rows and bytes
before and after (table + store + neg_train, by capacity) and the checkpoint file size are recorded with the times.
Prints one JSON line and writes it to --out.

  python tools/compact_timing.py [--repeats 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "compact.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel, compact_capacity
    shape = SHAPES[args.dataset]
    stream = make_stream(shape, seed=0)
    B, D, K = args.batch, 100, 10
    N, d = shape.num_nodes, shape.msg_dim
    E = stream.num_events if args.events is None else min(args.events, stream.num_events)
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
    old_tab, old_store = eng._tab, eng.model.store
    saved_eid, saved_ctl = eng.loader.e_id.clone(), eng.ctl.clone()

    def footprint(e):
        cap = e.event_capacity
        return {"rows": e.num_events, "capacity": cap,
                "bytes": int(sum(x.numel() * x.element_size() for x in e._tab) + e.model.store.numel() * 8
                             + e.neg_train.numel() * 8)}

    def restore():
        sync()
        eng._install_table(old_tab, E, old_store)
        eng.loader.e_id.copy_(saved_eid)
        eng.ctl.copy_(saved_ctl)
        sync()

    def leg_compact():
        restore()
        t0 = time.perf_counter()
        ws, n_live, n_arena, n_bad = eng._compact_plan(E)          # (ends in the host read of the record)
        t1 = time.perf_counter()
        assert n_bad == 0
        eng._drop_bindings()
        eng._compact_apply(ws, n_live, compact_capacity(n_live))
        sync()
        t2 = time.perf_counter()
        restore()
        t3 = time.perf_counter()
        eng.compact_events()
        sync()
        t4 = time.perf_counter()
        return {"compact_plan_ms": (t1 - t0) * 1e3, "compact_apply_ms": (t2 - t1) * 1e3,
                "compact_events_ms": (t4 - t3) * 1e3}

    def leg_replay():
        sync()
        t0 = time.perf_counter()
        e2 = build(events, E, params)
        sync()
        t1 = time.perf_counter()
        e2.observe_range(0, E, B)
        sync()
        t2 = time.perf_counter()
        e2.check()
        return {"replay_ms": (t2 - t0) * 1e3, "replay_observe_ms": (t2 - t1) * 1e3}, e2

    one = dict(src=np.zeros(1, np.int64), dst=np.zeros(1, np.int64), t=np.zeros(1, np.float32),
               msg=np.zeros((1, d), np.float32))
    tmp = tempfile.mkdtemp(prefix="tgnx_compact_")
    path = os.path.join(tmp, "stream.pt")

    def leg_load():
        sync()
        t0 = time.perf_counter()
        state = torch.load(path, map_location="cpu")
        t1 = time.perf_counter()
        e3 = build(one, 1, params)
        sync()
        t2 = time.perf_counter()
        e3.load_stream_state(state)
        sync()
        t3 = time.perf_counter()
        return {"load_file_ms": (t1 - t0) * 1e3, "load_ms": (t3 - t2) * 1e3, "load_with_engine_ms": (t3 - t0) * 1e3}, e3

    before = footprint(eng)
    leg_compact()                                              # warm-up of every leg; the state file for the load leg
    after = footprint(eng)
    t0 = time.perf_counter()
    torch.save(eng.stream_state(), path)
    save_ms = (time.perf_counter() - t0) * 1e3
    file_bytes = os.path.getsize(path)
    _, e2 = leg_replay()
    _, e3 = leg_load()
    # the three routes hold the same stream: memory and last_update bit for bit, the ring through kept
    restore()
    kept = eng.compact_events()
    sync()
    same = {"replay_memory": bool(torch.equal(e2.model.memory.memory, eng.model.memory.memory)),
            "replay_ring_through_kept": bool(torch.equal(
                kept[eng.loader.e_id[eng.loader.neighbors != -1]], e2.loader.e_id[e2.loader.neighbors != -1])),
            "load_memory": bool(torch.equal(e3.model.memory.memory, eng.model.memory.memory)),
            "load_ring": bool(torch.equal(e3.loader.e_id, eng.loader.e_id)),
            "load_table": bool(torch.equal(e3.msg, eng.msg) and torch.equal(e3.src, eng.src))}
    del e2, e3
    out = {"tool": "compact_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "ring": K,
           "batch": B, "events_observed": E, "before": before, "after": after, "state_file_bytes": file_bytes,
           "save_ms": round(save_ms, 3), "same_state": same,
           "unit": "ms per call, one call per window between device synchronisations (replay: one window of "
                   "ceil(E / B) observe steps); legs alternate within a repeat"}
    legs = {}
    for _ in range(args.repeats):
        for f in (leg_compact, leg_replay, leg_load):
            r = f()
            r = r[0] if isinstance(r, tuple) else r
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
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
