#!/usr/bin/env python3
"""Timing of node property prediction (csrc/tgnx_nodeprop.hip) on the same GPU and the same operands as the torch
composition a caller would write instead.  M = 1,000 label rows, D = 100, k = 10, C in {255, 513, 1001} (tgbn-token
has 1,001 classes); targets with 1-8 positive classes per row.

  row_eval / row_eval_torch     loss + NDCG@k of given logits: tgnx_node_loss_ndcg (one launch + the one-workgroup
                                mean) against F.cross_entropy(logits, y) + a torch NDCG (topk of the logits, gather,
                                topk of the targets; no tie averaging, which would cost torch a sort more)
  row_train / row_train_torch   the same plus dlogits: the row kernel writes them in the same pass; torch runs
                                autograd.grad of the loss
  head / head_torch             the whole head step — forward, soft cross-entropy, backward to every parameter and
                                to z — through tgnx.nn.NodePredictor + ops.soft_cross_entropy against torch.nn eager
                                (two Linear, relu, F.cross_entropy, backward)
  test_node                     tgnx.nodeprop.test_node over the validation rows of the wiki-shaped synthetic stream
                                (N = 9,227, 157,474 events, D = 100, batch 200, C = 255, labels from make_labels with
                                about --groups label times in the range): ms per label group, everything included
                                (observe_range between the groups, embed, head, the row kernel, the final host read)

Windowing as tools/similar_timing.py: a window is --iters calls between two device synchronisations after a warm-up
of the same shape; --repeats windows per leg, the legs alternating inside every repeat, all in one process.  Every
leg reports its windows, their median and range; the ratios are torch median over tgnx median, as measured.  Prints one
JSON line and writes it to --out.

  python tools/nodeprop_timing.py [--iters 300] [--repeats 5] [--groups 8] [--commit ID] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # the product's runtime configuration (tgnx/__init__.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--classes", default="255,513,1001")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "nodeprop.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tgb-tgn-dgl_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.nn.functional as F

    from tgnx import ops
    from tgnx.nn import NodePredictor
    assert torch.cuda.is_available(), "nodeprop_timing needs a GPU"
    dev = torch.device("cuda:0")
    M, D, k = args.rows, 100, args.k
    ns = ops.load()
    out = {"tool": "nodeprop_timing", "commit": args.commit, "device": torch.cuda.get_device_name(0), "rows": M, "D": D,
           "k": k, "iters": args.iters, "repeats": args.repeats, "unit": "ms per call", "shapes": {}}
    disc = (1.0 / torch.log2(torch.arange(2, k + 2, dtype=torch.float64, device=dev)))

    def torch_ndcg(logits, y):
        kk = min(k, logits.size(1))
        top = torch.topk(logits, kk, dim=1).indices
        dcg = (y.gather(1, top).double() * disc[:kk]).sum(1)
        idcg = (torch.topk(y, kk, dim=1).values.double() * disc[:kk]).sum(1)
        return torch.where(idcg > 0, dcg / idcg, torch.zeros_like(idcg))

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    for C in (int(c) for c in args.classes.split(",")):
        rng = np.random.default_rng(C)
        y = np.zeros((M, C), dtype=np.float32)
        for i in range(M):
            nz = rng.choice(C, size=int(rng.integers(1, 9)), replace=False)
            cnt = rng.integers(1, 6, size=nz.shape[0]).astype(np.float32)
            y[i, nz] = cnt / cnt.sum()
        y = torch.from_numpy(y).to(dev)
        z = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32)).to(dev)
        torch.manual_seed(C)
        mine = NodePredictor(D, C).to(dev)
        ref = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.ReLU(), torch.nn.Linear(D, C)).to(dev)
        ref[0].load_state_dict(mine.lin_node.state_dict())
        ref[2].load_state_dict(mine.out.state_dict())
        with torch.no_grad():
            logits = mine(z).contiguous()
        cum = ops._cum_on(k, dev)
        lg = logits.clone().requires_grad_(True)
        zg = z.clone().requires_grad_(True)
        params_m, params_r = list(mine.parameters()), list(ref.parameters())

        def row_train_torch():
            loss = F.cross_entropy(lg, y)
            return torch.autograd.grad(loss, lg)[0], torch_ndcg(logits, y)

        def head_mine():
            return torch.autograd.grad(ops.soft_cross_entropy(mine(zg), y), [zg] + params_m)

        def head_torch():
            return torch.autograd.grad(F.cross_entropy(ref(zg), y), [zg] + params_r)

        legs = {
            "row_eval": lambda: ns.node_loss_ndcg(logits, y, cum, k, True, False, True),
            "row_eval_torch": lambda: (F.cross_entropy(logits, y), torch_ndcg(logits, y)),
            "row_train": lambda: ns.node_loss_ndcg(logits, y, cum, k, True, True, True),
            "row_train_torch": row_train_torch,
            "head": head_mine,
            "head_torch": head_torch}
        # the two sides agree before they are timed (the NDCGs only where no score ties: torch's ignores them)
        a, b = legs["row_train"](), row_train_torch()
        res = {"max_dlogits_diff": float((a[2] - b[0]).abs().max()),
               "loss_diff": float((a[0] - F.cross_entropy(logits, y)).abs()),
               "max_ndcg_diff": float((a[3] - b[1]).abs().max())}
        ga, gb = head_mine(), head_torch()
        res["max_head_grad_diff"] = max(float((x - w).abs().max()) for x, w in zip(ga, gb))
        for n, fn in legs.items():
            window(fn, max(args.iters // 10, 3))                   # warm-up: allocator, first launches
            res[n] = {"windows": []}
        for _ in range(args.repeats):
            for n, fn in legs.items():
                res[n]["windows"].append(round(window(fn, args.iters), 4))
        for n in legs:
            w = res[n]["windows"]
            res[n].update(median=round(statistics.median(w), 4), min=min(w), max=max(w))
        for n in ("row_eval", "row_train", "head"):
            res[n + "_torch_over_tgnx"] = round(res[n + "_torch"]["median"] / res[n]["median"], 3)
        out["shapes"][str(C)] = res

    # ------------------------------------------------------------------ test_node per label group
    from tgnx.nodeprop import label_schedule, make_labels, test_node
    from tgnx.sampler import LastNeighborLoader
    from tgnx.synth import SHAPES, make_stream
    from tgnx.tgn import TgnAdam, TgnEngine, TGNModel
    shape = SHAPES["tgbl-wiki"]
    s = make_stream(shape, seed=0)
    B, C = 200, 255
    model = TGNModel(shape.num_nodes, s.num_events, shape.msg_dim, D, dev, ring=10, max_batch=B, max_neg=1, aggr="last",
                     dropout=0.1, generator=torch.Generator().manual_seed(0))
    loader = LastNeighborLoader(shape.num_nodes, 10, device=dev)
    eng = TgnEngine(model, loader, dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg),
                    TgnAdam(model, 1e-4), dst_nodes=np.unique(s.dst), seed=1234)
    eng._mode_train = False
    model._tgnx_engine = eng
    lo, hi = s.train_end, s.val_end
    labels = make_labels(s, C, (s.t[hi - 1] - s.t[lo]) / args.groups)
    sched = label_schedule(s.t.astype(np.float32), labels, lo, hi)
    head = NodePredictor(D, C).to(dev)
    eng.reset_state()
    eng.observe_range(0, lo, B)
    torch.cuda.synchronize()
    ld = eng.loader
    state = [model.memory.memory, model.memory.last_update, model.store, model.node_gen, ld.neighbors, ld.e_id, ld.t,
             eng.ctl]
    saved = [x.clone() for x in state]
    wins, res = [], None
    for r in range(args.loop_repeats + 1):                          # (the first pass is the warm-up)
        for x, w in zip(state, saved):
            x.copy_(w)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = test_node(model, loader, head, labels, lo, hi, batch=B, k=k)
        torch.cuda.synchronize()
        if r:
            wins.append(round((time.perf_counter() - t0) * 1e3 / max(res["groups"], 1), 4))
    out["test_node"] = {"dataset": "tgbl-wiki (synthetic)", "events": hi - lo, "batch": B, "classes": C,
                        "groups": res["groups"], "rows": res["rows"], "scheduled": len(sched), "ndcg": res["ndcg"],
                        "unit": "ms per label group (observe + embed + head + row kernel)", "windows": wins,
                        "median": round(statistics.median(wins), 4), "min": min(wins), "max": max(wins)}
    eng.check()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
