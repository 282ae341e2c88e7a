"""Per-call time of tgnx.nn.TGNMemory at tgbl-wiki's shape (N = 9,227, d = 172, D = T = 100, B = 200) on a synthetic
stream (tgnx/synth.py): forward(n_id) in training mode and update_state, each between a pair of device events
(so a call's own device -> host size read is inside its time), `--iters` iterations after `--warmup`.  One JSON
line.  The launch count per call comes from a separate profiled pass (torch.profiler's device kernel events), not
from the timed loop.

    python tools/memory_module_timing.py                 # the HIP module on the GPU
    python tools/memory_module_timing.py --cpu-oracle    # oracle/tgn_ref.RefTGNMemory on this machine's CPU (host clock)

The two are not like for like: a CPU restatement of the reference's Python loops against the device module."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, D_MSG, D_MEM, B = 9227, 172, 100, 200


def batches(n_batches, seed=0):
    from tgnx.synth import make_stream
    s = make_stream("tgbl-wiki", seed=seed, num_events=n_batches * B, num_nodes=N, msg_dim=D_MSG)
    rng = np.random.default_rng(seed + 1)
    for i in range(n_batches):
        sl = slice(i * B, (i + 1) * B)
        src, dst = torch.from_numpy(s.src[sl]), torch.from_numpy(s.dst[sl])
        neg = torch.from_numpy(rng.choice(s.dst_nodes, size=B))
        yield src, dst, torch.from_numpy(s.t[sl].astype(np.int64)), torch.from_numpy(s.msg[sl]), \
            torch.cat([src, dst, neg]).unique()


def stats(xs):
    xs = sorted(xs)
    return dict(median_us=round(statistics.median(xs) * 1e3, 1), p10_us=round(xs[len(xs) // 10] * 1e3, 1),
                p90_us=round(xs[(9 * len(xs)) // 10] * 1e3, 1))


def run_gpu(args):
    from tgnx import nn as tnn
    if not torch.cuda.is_available():
        raise SystemExit("memory_module_timing: no HIP device (use --cpu-oracle for the CPU restatement)")
    dev = torch.device("cuda")
    mem = tnn.TGNMemory(N, D_MSG, D_MEM, D_MEM, tnn.IdentityMessage(D_MSG, D_MEM, D_MEM),
                        tnn.LastAggregator()).to(dev).train()
    data = [tuple(x.to(dev) for x in b) for b in batches(args.warmup + args.iters + 1)]
    fwd, upd = [], []
    for i, (src, dst, t, msg, n_id) in enumerate(data[:-1]):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        z, _ = mem(n_id)
        e[1].record()
        e[2].record()
        mem.update_state(src, dst, t, msg)
        e[3].record()
        torch.cuda.synchronize()
        del z
        if i >= args.warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            upd.append(e[2].elapsed_time(e[3]))
    out = dict(tool="memory_module_timing", side="gpu module", device=torch.cuda.get_device_name(0), N=N, d=D_MSG,
               D=D_MEM, B=B, iters=args.iters, warmup=args.warmup, mean_n_id=round(float(np.mean(
                   [b[4].numel() for b in data[args.warmup:-1]])), 1),
               forward=stats(fwd), update_state=stats(upd), log_capacity=int(mem._log_src.numel()))
    # launches per call: one profiled call of each, after the timed loop
    src, dst, t, msg, n_id = data[-1]
    try:
        from torch.profiler import ProfilerActivity, profile

        def launches(fn):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [x for x in prof.events() if x.device_type == torch.autograd.DeviceType.CUDA]
            return len(ev), sum("memstore" in x.name for x in ev)
        out["forward_launches"], out["forward_memstore_launches"] = launches(lambda: mem(n_id))
        out["update_state_launches"], out["update_state_memstore_launches"] = launches(
            lambda: mem.update_state(src, dst, t, msg))
    except Exception as exc:  # a profiler that cannot trace this device: the times above stand, the count is absent
        out["launches"] = f"not measured ({type(exc).__name__}: {exc})"
    print(json.dumps(out))


def run_cpu_oracle(args):
    from oracle.tgn_ref import RefTGNMemory
    torch.manual_seed(0)
    mem = RefTGNMemory(N, D_MSG, D_MEM, D_MEM, aggr="last", updater="gru").train()
    fwd, upd = [], []
    for i, (src, dst, t, msg, n_id) in enumerate(batches(args.warmup + args.iters)):
        t0 = time.perf_counter()
        mem(n_id)
        t1 = time.perf_counter()
        mem.update_state(src, dst, t, msg)
        t2 = time.perf_counter()
        if i >= args.warmup:
            fwd.append((t1 - t0) * 1e3)
            upd.append((t2 - t1) * 1e3)
    print(json.dumps(dict(tool="memory_module_timing", side="cpu oracle (RefTGNMemory)", threads=torch.get_num_threads(),
                          N=N, d=D_MSG, D=D_MEM, B=B, iters=args.iters, warmup=args.warmup, forward=stats(fwd),
                          update_state=stats(upd))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-oracle", action="store_true")
    a = ap.parse_args()
    run_cpu_oracle(a) if a.cpu_oracle else run_gpu(a)
