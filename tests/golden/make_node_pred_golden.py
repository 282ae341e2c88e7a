"""Capture node_pred.npz from the reference's own NodePredictor (run where the reference checkout exists).

    python tests/golden/make_node_pred_golden.py --ref <reference checkout>

modules/decoder.py:30-41 (NodePredictor; the module imports torch only) is executed on seeded inputs with torch's
soft-target cross-entropy, and the numbers are written next to this script.  Nothing from the reference (source or
bytecode) is copied; only numbers:

  sd.<name>      the state dict (lin_node.weight [100, 100], lin_node.bias, out.weight [65, 100], out.bias)
  z [67, 100]    node embeddings;  y [67, 65] soft targets (sparse class histograms; row 5 is all zero, rows 6-8 do
                 not sum to 1)
  logits         NodePredictor(100, 65)(z)
  loss           F.cross_entropy(logits, y) (probability targets, mean over rows)
  grad.<name>    every parameter's gradient of the loss;  dz its gradient with respect to z
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference (cseduashraful/tgb-tgn-dgl)")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_decoder", os.path.join(a.ref, "modules", "decoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(23)
    M, D, C = 67, 100, 65
    head = mod.NodePredictor(D, C)
    rng = np.random.default_rng(23)
    z = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32)).requires_grad_(True)
    y = np.zeros((M, C), dtype=np.float32)
    for i in range(M):
        nz = rng.choice(C, size=int(rng.integers(1, 9)), replace=False)
        cnt = rng.integers(1, 6, size=nz.shape[0]).astype(np.float32)
        y[i, nz] = cnt / cnt.sum()
    y[5] = 0.0
    y[6:9] *= np.array([[0.5], [2.0], [3.25]], dtype=np.float32)
    logits = head(z)
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y))
    loss.backward()
    out = {"z": z.detach().numpy(), "y": y, "logits": logits.detach().numpy(), "loss": loss.detach().numpy(),
           "dz": z.grad.numpy()}
    for n, p in head.named_parameters():
        out["sd." + n] = p.detach().numpy()
        out["grad." + n] = p.grad.numpy()
    np.savez(os.path.join(HERE, "node_pred.npz"), **out)
    print({k: v.shape for k, v in out.items()}, float(loss.detach()))


if __name__ == "__main__":
    main()
