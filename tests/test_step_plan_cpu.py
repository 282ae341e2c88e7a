"""The train step's launch plan (tgnx_tgn_step_plan: host only) against tests/golden/step_plan.json, the launches the
step issued on an MI355X before the plan existed (a kernel trace of every train entry point over the configs below,
reduced by tools/step_plan_golden.py: label, grid, workgroup size and kernel instance per launch).  Every case sits
where a placement decision flips: the nine entry points (world 1 and the world-2 share), prepared or not, parity 0 /
1; 1 / 2 hops, GRU / RNN, DyRep embedding messages, last / mean aggregation (msg_dim 172 and 200: tgn_agg_emit<-1>);
ring 4 / 10 / 32 (the ring-10 predictor and attention backward; ring > 16 drops the per-event slot lists); with and
without the plan table and gather-ahead; batch 8 / 200 / 600 / 1100 / 2048 (1, 3, 5, 8 plan partitions: the plans
ride in the predictor launch for 2..4); 70 / 257 nodes and 16352 | 16353, 65504 | 65505 nodes (512 | 513 bitmap words:
the 2-words-per-thread walk; 2048 | 2049: the direct walk's threshold).

A kernel trace reports a launch's static LDS segment only, so the golden cannot hold the dynamic LDS bytes; the plan's
are compared with the sizes restated below from the kernels' own layout (tgn_scan_smem, tgn_pred_smem, the mark
bitmap, the walk's centre staging)."""
import ctypes
import json
import os

import pytest

from conftest import ROOT

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "step_plan.json")))
STEPS = []   # (case, launches)
for _c, _m, _pf, _par, _l in GOLD["cases"]:
    _mode, _world = GOLD["modes"][_m]
    STEPS.append((dict(zip(GOLD["config_fields"], GOLD["configs"][_c]), mode=_mode, world=_world, prefetched=_pf,
                       parity=_par), GOLD["launch_lists"][_l]))
MODES = {   # entry point -> (fuse_adam, world, pipelined, caller_scans, parity sets)
    "fwd_bwd": (0, 0, 0, 0, 0), "step": (1, 0, 0, 0, 0), "step_resident": (1, 1, 0, 0, 0),
    "step_pipelined": (1, 1, 1, 0, 0), "step_pp": (1, 1, 1, 0, 1), "fwd_bwd_resident": (0, 2, 0, 0, 0),
    "fwd_bwd_pipelined": (0, 2, 1, 0, 0), "fwd_bwd_split": (0, 2, 1, 1, 0), "fwd_bwd_pp": (0, 2, 1, 0, 1)}


def _plan(cs):
    from tgnx import _lib
    from tgnx.tgn import TgnConfig
    cfg = TgnConfig(num_nodes=cs["N"], num_events=3 * cs["B"], ring=cs["ring"], mem_dim=cs["D"], msg_dim=cs["d"], heads=2,
                    max_batch=cs["B"], max_neg=1, aggr=0 if cs["aggr"] == "last" else 1, dropout=0.1, lr=1e-4, beta1=0.9,
                    beta2=0.999, eps=1e-8, layers=cs["layers"], updater=1 if cs["updater"] == "rnn" else 0,
                    emb_in_msg=cs["emb"])
    fuse, world, pipelined, caller_scans, pp = MODES[cs["mode"]]
    assert world == (0 if cs["mode"] in ("fwd_bwd", "step") else cs["world"])
    prefetch = 0 if not pipelined else 1 if cs["prefetched"] else 2          # TGNX_TGN_PREFETCH_*
    assert (cs["parity"] >= 0) == bool(pp)
    out = (_lib.TgnLaunch * len(_lib.STEP_LABELS))()
    rc = _lib.lib().tgnx_tgn_step_plan(ctypes.byref(cfg), fuse, world, prefetch, caller_scans, cs["parity"],
                                      1 if world == 2 else 0, 1 if cs["ptab"] and world else 0, 0 if cs["ga"] else 2, out)
    assert rc == 0, _lib.lib().tgnx_last_error()
    return list(out)


def _scan_smem(B):
    n = 1
    while n < 2 * B:
        n *= 2
    return n * 16 + (2 * B + 4) * 4 + 64


def _dynamic_lds(cs, launches, labels):
    """label -> the dynamic LDS bytes its launch must ask for, from the kernels' layout and the traced launches"""
    _, _, pipelined, _, pp = MODES[cs["mode"]]
    Bk = -(-cs["B"] // max(cs["world"], 1))                              # the rank's share of the batch
    by = {labels[l[0]]: l for l in launches}
    out = {name: _scan_smem(cs["B"]) for name in ("tgn_scan", "tgn_scan_early", "tgn_scan_next") if name in by}
    # the predictor: its staged weights; a pipelined step's mark blocks ride in it (3 bitmaps of 2048 words); so do
    # the plan blocks when more workgroups ride than the mark blocks and the one sort block
    D = cs["D"]
    nmk = -(-3 * Bk * 16 // 256) if pipelined else 0
    riders = by["tgn_pred_train"][1] - Bk - nmk
    out["tgn_pred_train"] = max(2 * D * (D + 1) * 4, 3 * 2048 * 4 if nmk else 0, _scan_smem(cs["B"]) if riders > 1 else 0)
    # a parity-set step scans the next batch somewhere: as a ScanJob (kernel 1 of the dz0 / dW_cell launch), in its
    # own launch, or else as the walk block of the attention backward, which stages the rank's 3 B centres
    elsewhere = by["tgn_wgrad_dz0"][3] or by["tgn_wgrad3"][3] or "tgn_scan_early" in by
    if pp and not elsewhere:
        out["tgn_attn_bwd"] = 3 * Bk * 12 + 16
    return out


def test_golden_covers_the_decisions():
    cases = [cs for cs, _ in STEPS]
    assert {c["mode"] for c in cases} == set(MODES)
    for key, vals in (("layers", {1, 2}), ("updater", {"gru", "rnn"}), ("emb", {0, 3}), ("aggr", {"last", "mean"}),
                      ("ring", {4, 10, 32}), ("ptab", {0, 1}), ("ga", {0, 1}), ("world", {1, 2}), ("prefetched", {0, 1}),
                      ("parity", {-1, 0, 1}), ("d", {16, 172, 200})):
        assert vals <= {c[key] for c in cases}, key
    assert {8, 200, 2048} <= {c["B"] for c in cases}
    assert {70, 257, 16352, 16353, 65504, 65505} <= {c["N"] for c in cases}
    labels = GOLD["labels"]
    seen = {labels[l[0]] for ls in GOLD["launch_lists"] for l in ls}
    assert seen == set(labels), set(labels) - seen                     # every launch of the step occurs somewhere


@pytest.mark.parametrize("mode", sorted(MODES))
def test_step_plan_matches_the_traced_launches(mode):
    from tgnx import _lib
    labels = list(_lib.STEP_LABELS)
    assert labels == GOLD["labels"]
    n = 0
    for cs, launches in STEPS:
        if cs["mode"] != mode:
            continue
        recs = _plan(cs)
        assert [r.label for r in recs] == list(range(len(labels)))
        got = [[r.label, r.grid, r.block, r.kernel] for r in recs if r.issued]
        assert got == launches, cs
        lds = _dynamic_lds(cs, launches, labels)
        for r in recs:
            if not r.issued:
                assert (r.grid, r.block, r.lds, r.kernel) == (0, 0, 0, 0), (cs, labels[r.label])
            else:
                assert r.lds == lds.get(labels[r.label], 0), (cs, labels[r.label], r.lds)
        n += 1
    assert n >= 40
