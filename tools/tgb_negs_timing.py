#!/usr/bin/env python3
"""Timing and effect of the device hist_rnd evaluation negatives at the wiki shape: the synthetic tgbl-wiki stream
(N = 9,227 nodes, 157,474 events), its validation split, k = 999 negatives per event.

Two steps, each a fresh child process under its own time limit; the second runs only if the first succeeded:

  timing   PairHistory.build over the whole stream and tgb_negatives over the validation split (index given; the
           status read included), one call per window between two device synchronisations after a warm-up, against
           two host baselines on the same box: tgb_io.uniform_negatives for the same split (what the loaders use
           when no table comes with the data), and a numpy version of TGB's per-event procedure (per event a
           setdiff1d over the pool for the random part and over the source's history for the historical part) on the
           first `--slice` events of the split only — reported per slice and per event, not extrapolated
  mrr      one training epoch of the drop-in loop, then the validation MRR of that model under the loader's uniform
           negatives and under hist_rnd negatives (same state restored before each pass), and EdgeBank-inf's MRR
           under both tables

Prints one JSON line and writes it to --out.

  python tools/tgb_negs_timing.py [--repeats 7] [--slice 2000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)

K = 999
LIMITS = {"timing": 300, "mrr": 420}                            # seconds per step


def numpy_tgb_slice(src, dst, t, lo, hi, n, k, pool, rng):
    """TGB's per-event generation (negative_generator.py, hist_rnd) restated with numpy for rows [lo, lo + n): the
    split's same-time positives are looked up per (source, timestamp) key, the historical candidates are the
    source's pre-split destinations minus them, the random ones a setdiff1d of the pool against both."""
    import numpy as np
    hist = {}
    for s, d in zip(src[:lo].tolist(), dst[:lo].tolist()):
        hist.setdefault(s, set()).add(d)
    hist = {s: np.fromiter(v, np.int64, len(v)) for s, v in hist.items()}
    now = {}
    for s, d, ts in zip(src[lo:hi].tolist(), dst[lo:hi].tolist(), t[lo:hi].tolist()):
        now.setdefault((s, ts), []).append(d)
    out = np.empty((n, k), np.int64)
    q = k // 2
    for r in range(n):
        s = int(src[lo + r])
        pos = np.unique(now[(s, float(t[lo + r]))])
        h = np.setdiff1d(hist.get(s, np.empty(0, np.int64)), pos)
        kh = min(q, h.size)
        out[r, :kh] = rng.choice(h, kh, replace=False) if kh else []
        valid = np.setdiff1d(pool, np.union1d(hist.get(s, np.empty(0, np.int64)), pos))
        out[r, kh:] = rng.choice(valid, k - kh, replace=valid.size < k - kh)
    return out


def step_timing(args):
    import numpy as np
    import torch

    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgb_io import uniform_negatives
    from tgnx.tgb_negs import PairHistory, hist_rnd, tgb_negatives
    s = make_stream(SHAPES[args.dataset], seed=0)
    lo, hi, E = int(s.train_end), int(s.val_end), int(s.num_events)
    dev = torch.device("cuda:0")
    src, dst = torch.from_numpy(s.src).to(dev), torch.from_numpy(s.dst).to(dev)
    t = torch.from_numpy(np.asarray(s.t, np.float64)).to(dev)
    pool_np = np.unique(s.dst)
    pool = torch.from_numpy(pool_np).to(dev)
    N = int(max(s.src.max(), s.dst.max())) + 1

    def window(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    legs = {"index_build_ms": lambda: PairHistory.build(src, dst, N),
            "generate_ms": lambda: tgb_negatives(src, dst, t, lo, hi, K, pool=pool, seed=1, index=idx, return_info=True),
            "generate_kernels_ms": lambda: hist_rnd(src, dst, t, lo, hi, K, K // 2, lo, pool, idx, seed=1)}
    idx = PairHistory.build(src, dst, N)
    times = {k: [] for k in legs}
    for f in legs.values():                                         # warm-up of every leg
        window(f)
    for _ in range(args.repeats):
        for name, f in legs.items():
            times[name].append(round(window(f)[0], 3))
    negs, k_hist, status = legs["generate_ms"]()
    t0 = time.perf_counter()
    uni = uniform_negatives(s.dst, lo, hi, K, seed=1)
    uniform_ms = (time.perf_counter() - t0) * 1e3
    n_slice = min(args.slice, hi - lo)
    t0 = time.perf_counter()
    numpy_tgb_slice(s.src, s.dst, np.asarray(s.t, np.float64), lo, hi, n_slice, K, pool_np, np.random.default_rng(0))
    slice_ms = (time.perf_counter() - t0) * 1e3
    return {"num_nodes": N, "num_events": E, "split": [lo, hi], "k": K, "pool": int(pool_np.size), "nnz": idx.nnz,
            "k_hist_mean": float(k_hist.double().mean()), "k_hist_max": int(k_hist.max()), "status": status,
            "uniform_positive_hits": int((uni == s.dst[lo:hi, None]).sum()), **times,
            "median": {k: float(np.median(v)) for k, v in times.items()},
            "host_uniform_negatives_ms": round(uniform_ms, 1),
            "host_numpy_tgb_slice_events": n_slice, "host_numpy_tgb_slice_ms": round(slice_ms, 1),
            "host_numpy_tgb_ms_per_event": round(slice_ms / max(n_slice, 1), 4),
            "device_generate_ms_per_event": float(np.median(times["generate_ms"]) / max(hi - lo, 1))}


def step_mrr(args):
    import torch

    import pyg_epoch_utils as pe
    import pyg_model_utils as pm
    from tgnx.data import getDataWithDependecyBlock
    from tgnx.neg import NegLinkSamplerDest
    from tgnx.sampler import LastNeighborLoader
    os.environ["TGNX_EVAL_NEGS"] = str(K)
    data, tr, va, te, ns, ev, metric = getDataWithDependecyBlock(args.dataset, {"batch_size": 200})
    d, D, N = data.msg.shape[1], 100, data.num_nodes
    torch.manual_seed(0)
    model = pm.getModel(d, D, N, "cuda", ring=10, max_batch=200, dropout=0.1)
    opt = pm.getOptimizer(model, 1e-4)
    nl = LastNeighborLoader(N, 10, device="cuda")
    nds = NegLinkSamplerDest(torch.unique(data.dst), device="cuda")
    crit = torch.nn.BCEWithLogitsLoss()
    loss = pe.train(model, data.msg, tr, nl, nds, None, "cuda", opt, crit)
    eng = model["model"]._tgnx_engine
    eng.finish()
    torch.cuda.synchronize()
    m = eng.model
    held = [(x, x.clone()) for x in (m.flat, m.memory.memory, m.memory.last_update, m.store, m.node_gen, nl.neighbors,
                                      nl.e_id, nl.t, nl._assoc, eng.ctl)]

    def val_mrr():
        torch.cuda.synchronize()
        with torch.no_grad():
            for x, saved in held:
                x.copy_(saved)
        nl.cur_e_id = tr.hi
        eng.invalidate_prefetch()
        eng._mode_train = True                                     # test() flushes the stored messages again
        return pe.test(model, data.msg, va, nl, ns, None, "cuda", opt, crit, ev, metric, "val")
    out = {"train_loss": float(loss), "val_events": va.hi - va.lo}
    out["val_mrr_uniform"] = val_mrr()
    out["edgebank_mrr_uniform"] = pe.edgebank(va)
    pe.tgb_negatives(va, K, seed=1)
    out["val_mrr_hist_rnd"] = val_mrr()
    out["edgebank_mrr_hist_rnd"] = pe.edgebank(va)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="tgbl-wiki")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slice", type=int, default=2000, help="events of the split the numpy TGB baseline generates for")
    ap.add_argument("--step", choices=list(LIMITS), default=None, help="run one step in this process (the driver does)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "tgb_negs.json"))
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"timing": step_timing, "mrr": step_mrr}[args.step](args)))
        return 0
    out = {"tool": "tgb_negs_timing", "dataset": args.dataset,
           "unit": "ms per call, one call per window between device synchronisations, legs alternating within a repeat; "
                   "host_* are single host-clock runs of numpy code on the same box"}
    for step, limit in LIMITS.items():                              # chained: a failed or timed-out step ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--dataset", args.dataset, "--repeats",
               str(args.repeats), "--slice", str(args.slice)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"tgb_negs_timing: step {step} exceeded {limit} s; stopping", file=sys.stderr)
            return 124
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"tgb_negs_timing: step {step} failed ({r.returncode}); stopping", file=sys.stderr)
            return r.returncode or 1
        out[step] = json.loads(res[-1][len("RESULT "):])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
