#!/usr/bin/env python3
"""Timing of node-space growth at the wiki shape: N = 9,227 nodes, msg_dim 172, D = 100, ring 10, B = 200, with HALF
the synthetic stream (78,737 of 157,474 events) observed on a reset engine.  All legs in one process on one device,
alternating within a repeat; every leg starts from a fresh engine that loaded the same stream_state() snapshot, and
every window lies between two device synchronisations, after one warm-up pass of every leg.

  grow_1 / grow_1p5x / grow_2x   ONE TgnEngine.grow_nodes call: to N + 1, to 1.5 N, to 2 N (row tensors reallocated and
              copied, store re-laid, fresh workspace, the host read of the bad-run count)
  grow_in_capacity   one grow_nodes(N + 1) after reserve_nodes(2 N): the store re-lay and the fresh workspace alone
  auto        observe_events(grow=True) over `--auto-batches` batches of B events, each naming ONE node the engine has
              not seen (capacity by grown_node_capacity), against the same batches with that id folded back into
              [0, N) and grow=False: `auto_per_new_node_ms` is the difference per batch
  rebuild     the route before this tool's feature: a new model + engine at N + 1 nodes over a one-row table and
              load_stream_state of the snapshot padded on the host (the padding and the host-to-device copies
              included; `state_to_host_ms`, the snapshot's device-to-host copy that route also needs, is apart)
  replay      the route before checkpoints: a new model + engine at N + 1 over the history and observe_range over it
  first_observe / steady_observe   the first observe() of B rows after a growth (fresh workspace, bindings remade)
              against the mean of the following `--steady` observes

Prints one JSON line and writes it to --out.

  python tools/grow_timing.py [--repeats 3] [--out FILE]
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

RESET_ROW = {"memory": 0, "last_update": 0, "node_gen": 0, "store_nodes": 0, "neighbors": -1, "e_id": -1, "ring_t": -1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--events", type=int, default=None, help="observe only this many rows (default: half the stream)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--auto-batches", type=int, default=64)
    ap.add_argument("--steady", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "grow.json"))
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
    nab = args.auto_batches
    assert E + (nab + args.steady + 2) * B <= stream.num_events
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)

    def rows(lo, hi):
        return dict(src=stream.src[lo:hi], dst=stream.dst[lo:hi], t=stream.t[lo:hi].astype(np.float32),
                    msg=stream.msg[lo:hi])

    history = rows(0, E)
    one = rows(0, 1)
    params = None

    def build(ev, n_nodes):
        model = TGNModel(n_nodes, int(ev["src"].shape[0]), d, D, dev, ring=K, max_batch=B, max_neg=1, aggr="last",
                         dropout=0.1, generator=gen)
        if params is not None:
            model.flat.copy_(params)
        eng = TgnEngine(model, LastNeighborLoader(n_nodes, K, device=dev), ev, TgnAdam(model, 1e-4), seed=1234)
        eng.reset_state()
        return eng

    def sync():
        torch.cuda.synchronize()

    base = build(history, N)
    params = base.model.flat.clone()
    base.observe_range(0, E, B)
    sync()
    base.check()
    snap = base.stream_state()
    sync()
    t0 = time.perf_counter()
    snap_host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in snap.items()}
    state_to_host_ms = (time.perf_counter() - t0) * 1e3

    def fresh():
        e = build(one, N)
        e.load_stream_state(snap)
        sync()
        return e

    def timed(f):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def leg_grow():
        out = {}
        for name, n in (("grow_1_ms", N + 1), ("grow_1p5x_ms", N + N // 2), ("grow_2x_ms", 2 * N)):
            e = fresh()
            out[name] = timed(lambda: e.grow_nodes(n))
            assert int(e.cfg.num_nodes) == n
        e = fresh()
        e.reserve_nodes(2 * N)
        out["grow_in_capacity_ms"] = timed(lambda: e.grow_nodes(N + 1))
        return out

    def auto_rows(i, new):
        r = {k: np.array(v, copy=True) for k, v in rows(E + i * B, E + (i + 1) * B).items()}
        r["dst"][B // 2] = N + i if new else (N + i) % N
        return r

    def leg_auto():
        out = {}
        for name, new in (("auto_grow_ms", True), ("auto_plain_ms", False)):
            e = fresh()
            chunks = [auto_rows(i, new) for i in range(nab)]

            def run():
                for r in chunks:
                    e.observe_events(r["src"], r["dst"], r["t"], r["msg"], batch=B, grow=new)
            out[name] = timed(run)
            e.check()
            assert int(e.cfg.num_nodes) == (N + nab if new else N)
            if new:
                out["auto_capacity_end"] = e.node_capacity
        out["auto_per_new_node_ms"] = (out["auto_grow_ms"] - out["auto_plain_ms"]) / nab
        return out

    def pad_host(state, n1):
        n0 = int(state["num_nodes"])
        out = dict(state)
        out["num_nodes"] = n1
        for k, fill in RESET_ROW.items():
            x = state[k]
            out[k] = torch.cat([x, torch.full((n1 - n0,) + tuple(x.shape[1:]), fill, dtype=x.dtype)], 0)
        return out

    def leg_rebuild():
        sync()
        t0 = time.perf_counter()
        padded = pad_host(snap_host, N + 1)
        t1 = time.perf_counter()
        e = build(one, N + 1)
        e.load_stream_state(padded)
        sync()
        t2 = time.perf_counter()
        return {"rebuild_pad_ms": (t1 - t0) * 1e3, "rebuild_ms": (t2 - t0) * 1e3}, e

    def leg_replay():
        sync()
        t0 = time.perf_counter()
        e = build(history, N + 1)
        sync()
        t1 = time.perf_counter()
        e.observe_range(0, E, B)
        sync()
        t2 = time.perf_counter()
        e.check()
        return {"replay_ms": (t2 - t0) * 1e3, "replay_observe_ms": (t2 - t1) * 1e3}, e

    def leg_first_observe():
        e = fresh()
        r = rows(E, E + (args.steady + 1) * B)
        e.append_events(r["src"], r["dst"], r["t"], r["msg"])
        e.observe(E, B)                                        # (the appended table's first step: not the growth's cost)
        e.grow_nodes(N + 1)
        first = timed(lambda: e.observe(E + B, B))

        def run():
            for i in range(2, args.steady + 1):
                e.observe(E + i * B, B)
        steady = timed(run) / (args.steady - 1)
        e.check()
        return {"first_observe_ms": first, "steady_observe_ms": steady}

    # warm-up of every leg, and the three routes hold the same state
    g = fresh()
    g.grow_nodes(N + 1)
    _, e2 = leg_rebuild()
    _, e3 = leg_replay()
    sync()
    sg = g.stream_state()
    same = {}
    for name, e in (("rebuild", e2), ("replay", e3)):
        s = e.stream_state()
        same[name] = bool(all(torch.equal(sg[k], s[k]) for k in sg if torch.is_tensor(sg[k]) and k != "ctl"))
    del e2, e3, g
    leg_grow()
    leg_auto()
    leg_first_observe()
    m = base.model
    node_bytes = int(sum(x.numel() * x.element_size() for x in (m.memory.memory, m.memory.last_update, m.node_gen,
                                                                base.loader.neighbors, base.loader.e_id, base.loader.t,
                                                                base.loader._assoc)))
    out = {"tool": "grow_timing", "dataset": args.dataset, "num_nodes": N, "msg_dim": d, "mem_dim": D, "ring": K,
           "batch": B, "events_observed": E, "auto_batches": nab, "node_tensor_bytes": node_bytes,
           "store_bytes": int(m.store.numel() * 8), "ws_bytes": int(base.ws.numel()),
           "state_to_host_ms": round(state_to_host_ms, 3), "same_state": same,
           "unit": "ms per window between device synchronisations; one call per window except auto (auto_batches "
                   "observe_events calls), replay (ceil(E / B) observe steps) and steady_observe (mean of the steps "
                   "after the first); legs alternate within a repeat"}
    legs = {}
    for _ in range(args.repeats):
        for f in (leg_grow, leg_auto, leg_rebuild, leg_replay, leg_first_observe):
            r = f()
            r = r[0] if isinstance(r, tuple) else r
            for k, v in r.items():
                legs.setdefault(k, []).append(round(v, 4))
    out.update(legs)
    med = {k: float(np.median(v)) for k, v in legs.items()}
    out["median"] = med
    out["ratio"] = {"rebuild_over_grow_1": round(med["rebuild_ms"] / med["grow_1_ms"], 2),
                    "replay_over_grow_1": round(med["replay_ms"] / med["grow_1_ms"], 2),
                    "first_over_steady_observe": round(med["first_observe_ms"] / med["steady_observe_ms"], 2),
                    "grow_in_capacity_over_grow_1": round(med["grow_in_capacity_ms"] / med["grow_1_ms"], 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
