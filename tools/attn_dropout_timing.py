#!/usr/bin/env python3
"""Timing of the attention-dropout operator (tgnx.ops.edge_attention(dropout=0.1); csrc/tgnx_ops.hip attn_fwd /
attn_bwd <NR, DROP = true>) at a wiki-shaped call: H = 2 heads of C = 50 channels, 600 destinations, ring 10.

Shapes:
  sparse   degrees uniform in 0..7  (E about 2,100: rings partly filled)
  full     every ring full          (E = 6,000)

Legs, all in one process on the same operands, alternating within a window:

  drop         the dropout operator at p = 0.1 (edge_attn_drop_fwd / _bwd), explicit int64 keys as a TGN loop passes
  drop_nokeys  the same with the default keys (no key loads)
  plain        the dropout-off operator (edge_attn_fwd / _bwd): the yardstick.  Its kernels are the DROP = false
               instantiations, whose results are bit-identical to the operator before dropout existed
  eager        a torch eager composition: scatter softmax (scatter_reduce amax, exp, index_add, divide), F.dropout,
               index_add of the weighted values

each as `fwd` (forward only, under no_grad) and `fwd_bwd` (forward, then torch.autograd.grad of out·dout with respect
to q, k, v, e).  A window is `--calls` calls of one leg between two device synchronisations, after a warm-up of
every leg; `--windows` windows per leg.  Prints one JSON line and writes it to --out.

  python tools/attn_dropout_timing.py [--windows 5] [--calls 300] [--out FILE]
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

H, C, N_DST, P, SEED = 2, 50, 600, 0.1, 20240607


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "attn_dropout.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    from tgnx.ops import edge_attention
    assert torch.cuda.is_available(), "attn_dropout_timing needs a GPU"
    dev = torch.device("cuda:0")

    def eager(q, k, v, e, i, p=P):
        kk, vv = (k + e).view(-1, H, C), (v + e).view(-1, H, C)
        a = (q[i].view(-1, H, C) * kk).sum(-1) / math.sqrt(C)
        idx = i.view(-1, 1).expand(-1, H)
        amax = torch.full((N_DST, H), -math.inf, device=dev).scatter_reduce(0, idx, a, "amax", include_self=True)
        ex = (a - amax[i]).exp()
        alpha = ex / (torch.zeros(N_DST, H, device=dev).index_add(0, i, ex) + 1e-16)[i]
        alpha = F.dropout(alpha, p=p, training=p > 0)
        return torch.zeros(N_DST, H, C, device=dev).index_add(0, i, vv * alpha.unsqueeze(-1)).view(N_DST, H * C)

    def window(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    shapes = {}
    for shape in ("sparse", "full"):
        rng = np.random.default_rng(26)
        deg = torch.from_numpy(rng.integers(0, 8, N_DST) if shape == "sparse" else np.full(N_DST, 10))
        E = int(deg.sum())
        g = torch.Generator().manual_seed(E)
        indptr = torch.zeros(N_DST + 1, dtype=torch.long)
        indptr[1:] = deg.cumsum(0)
        i = torch.repeat_interleave(torch.arange(N_DST), deg).to(dev)
        indptr = indptr.to(dev)
        q = torch.randn(N_DST, H * C, generator=g).to(dev).requires_grad_(True)
        k, v, e = (torch.randn(E, H * C, generator=g).to(dev).requires_grad_(True) for _ in range(3))
        dout = torch.randn(N_DST, H * C, generator=g).to(dev)
        dkey = torch.from_numpy(rng.permutation(9227)[:N_DST].astype(np.int64)).to(dev)
        ekey = torch.from_numpy(rng.permutation(157474)[:E].astype(np.int64)).to(dev)
        leaves = (q, k, v, e)
        fwd = {
            "drop": lambda: edge_attention(q, k, v, e, indptr, H, dropout=P, seed=SEED, dst_key=dkey, edge_key=ekey)[0],
            "drop_nokeys": lambda: edge_attention(q, k, v, e, indptr, H, dropout=P, seed=SEED)[0],
            "plain": lambda: edge_attention(q, k, v, e, indptr, H)[0],
            "eager": lambda: eager(q, k, v, e, i),
        }

        def no_grad(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def with_grad(f):
            return lambda: torch.autograd.grad(f(), leaves, dout)

        legs = {}
        for name, f in fwd.items():
            legs[f"{name}_fwd"] = no_grad(f)
            legs[f"{name}_fwd_bwd"] = with_grad(f)
        # same operands, same results: plain == drop at p = 0 bit for bit; the eager composition's softmax agrees
        with torch.no_grad():
            a = edge_attention(q, k, v, e, indptr, H)[0]
            b = edge_attention(q, k, v, e, indptr, H, dropout=0.0, seed=SEED)[0]
            c = eager(q, k, v, e, i, 0.0)
        assert torch.equal(a, b)
        eager_dev = float((a - c).abs().max())
        assert eager_dev < 1e-4, eager_dev
        for f in legs.values():                                    # warm-up of every leg
            for _ in range(3):
                f()
        times = {name: [] for name in legs}
        for _ in range(args.windows):
            for name, f in legs.items():
                times[name].append(round(window(f), 5))
        shapes[shape] = {"n_dst": N_DST, "edges": E, "eager_vs_plain_max_abs_dev_dropout_off": eager_dev, "ms": times,
                         "median_ms": {name: float(np.median(t)) for name, t in times.items()}}
    out = {"tool": "attn_dropout_timing", "heads": H, "channels": C, "p": P, "windows": args.windows,
           "calls_per_window": args.calls, "device": torch.cuda.get_device_name(0),
           "unit": "ms per call, `calls_per_window` calls of one leg between two device synchronisations (host clock); "
                   "fwd under no_grad, fwd_bwd = forward + torch.autograd.grad to q, k, v, e",
           "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
