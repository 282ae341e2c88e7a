"""Two eager train steps of every train entry point over a list of small configs, each step bracketed by a 1-block
ring_reset launch on scratch tensors (the separator), to be run under `rocprofv3 --kernel-trace` (no counters).
Writes <out dir>/cases.json: the ordered list of bracketed steps.  Case sets: `plan`, the configs of
tests/golden/step_plan.json (tools/step_plan_golden.py turns the trace into that file); `seq`, 257 nodes, batch 8 and
200, 1 and 2 hops (profiles/r21/launch_seq_*.txt).  TGNX_LIB selects the library.

    rocprofv3 --kernel-trace --output-format csv -d <dir>/prof -o run -- python tools/step_trace.py <dir> plan
    python tools/trace_launches.py <dir>/prof <dir>/launches.txt"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tgb-tgn-dgl_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tgnx import _lib  # noqa: E402
from tgnx.sampler import LastNeighborLoader  # noqa: E402
from tgnx.synth import make_stream  # noqa: E402
from tgnx.tgn import TgnAdam, TgnEngine, TGNModel, _p  # noqa: E402

BASE = dict(N=257, B=8, ring=10, layers=1, updater="gru", emb=0, aggr="last", d=16, D=32, ptab=1, ga=1)


def cfgs(which):
    def c(**kw):
        return dict(BASE, **kw)
    if which == "seq":
        return [c(B=b, layers=l) for b in (8, 200) for l in (1, 2)]
    out = [c(), c(layers=2), c(updater="rnn"), c(updater="rnn", layers=2), c(emb=3), c(aggr="mean", d=172),
           c(aggr="mean", d=200), c(ring=4), c(ring=32), c(ring=4, layers=2), c(ptab=0), c(ga=0), c(ptab=0, layers=2),
           c(B=200), c(B=200, layers=2), c(B=2048), c(B=2048, layers=2), c(N=70), c(N=70, B=200),
           c(B=200, ptab=0), c(B=600, ptab=0), c(B=1100, ptab=0), c(B=2048, ptab=0), c(B=600), c(B=1100)]
    for n in (16352, 16353, 65504, 65505):   # bitmap words 512 | 513, 2048 | 2049
        out += [c(N=n), c(N=n, B=200), c(N=n, ptab=0), c(N=n, B=200, ptab=0), c(N=n, layers=2)]
    out += [c(N=65505, B=2048), c(N=65505, B=2048, ptab=0), c(N=9227, B=200, d=172, D=100),
            c(N=9227, B=200, d=172, D=100, layers=2)]
    return out


MODES = ["fwd_bwd", "step", "step_resident", "step_pipelined", "step_pp", "fwd_bwd_resident", "fwd_bwd_pipelined",
         "fwd_bwd_split", "fwd_bwd_pp"]
W2 = {"fwd_bwd_resident", "fwd_bwd_pipelined", "fwd_bwd_split", "fwd_bwd_pp"}


def main(out, which):
    dev = torch.device("cuda")
    sep_e = torch.zeros(8, dtype=torch.long, device=dev)
    sep_t = torch.zeros(8, dtype=torch.float32, device=dev)

    def sep():
        _lib.call("tgnx_ring_reset", _lib.ptr(sep_e), _lib.ptr(sep_t), 1, 1, _lib.stream(dev))

    log = []
    engs = []
    for cf in cfgs(which):
        N, B = cf["N"], cf["B"]
        s = make_stream("tgbl-wiki", seed=5, num_events=3 * B, num_nodes=N, msg_dim=cf["d"])
        ev = dict(src=s.src, dst=s.dst, t=s.t.astype(np.float32), msg=s.msg)
        for mode in MODES:
            world = 2 if mode in W2 else 1
            if cf["emb"] and world == 2:
                continue   # (DyRep embedding messages are a world-1 step)
            torch.manual_seed(0)
            kw = dict(memory="dyrep", use_src_emb_in_msg=True, use_dst_emb_in_msg=True) if cf["emb"] else {}
            model = TGNModel(N, s.num_events, cf["d"], cf["D"], dev, ring=cf["ring"], max_batch=B, max_neg=1,
                             aggr=cf["aggr"], dropout=0.1, layers=cf["layers"], updater=cf["updater"], **kw)
            e = TgnEngine(model, LastNeighborLoader(N, cf["ring"], device=dev), ev, TgnAdam(model, 1e-3),
                          dst_nodes=s.dst_nodes, seed=7, rank=0, world=world)
            e.exchange = lambda comm, async_op: None
            engs.append(mode)
            e.use_plan_table = bool(cf["ptab"])
            e.gather_ahead = bool(cf["ga"])
            e.pipeline = mode not in ("step_resident", "fwd_bwd_resident")
            e.parity_sets = mode in ("step_pp", "fwd_bwd_pp")
            e.split_scan = mode == "fwd_bwd_split"
            if mode in ("fwd_bwd", "step"):
                e.reset_state()
                for st in range(2):
                    e.advance(st * B, B, True)
                    b = e._buffers(_p(e.neg_train))
                    sep()
                    _lib.call("tgnx_tgn_train_" + mode, ctypes.byref(e.cfg), ctypes.byref(b), 1, 1, e._stream())
                    sep()
                    log.append(dict(cf, mode=mode, world=world, step=st, prefetched=0, parity=-1))
                    if mode == "fwd_bwd":
                        e._pending = b
                        e.apply_update()
            else:
                e.bind_resident(0, 3 * B, B, dropout=True)
                e.begin_epoch()
                pre = e._pre

                def wrapped(prefetched=False, parity=None, apply=None, pre=pre, e=e, mode=mode, cf=cf, world=world):
                    sep()
                    pre(prefetched, parity, apply)
                    sep()
                    log.append(dict(cf, mode=mode, world=world, step=sum(1 for x in log if x.get("eng") == len(engs)),
                                    prefetched=1 if prefetched else 0, parity=e._parity if e._pp() else -1,
                                    eng=len(engs)))
                e._pre = wrapped
                for st in range(2):
                    e.resident_train_step()
                e.finish()
            torch.cuda.synchronize()
            e.check()
            del e, model
    for x in log:
        x.pop("eng", None)
    os.makedirs(out, exist_ok=True)
    json.dump(log, open(os.path.join(out, "cases.json"), "w"))
    print("steps", len(log))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
