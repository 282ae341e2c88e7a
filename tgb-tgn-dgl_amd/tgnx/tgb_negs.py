"""TGB-style `hist_rnd` evaluation negatives, generated on the device (include/tgnx.h tgnx_pair_index_* /
tgnx_negs_hist_rnd; csrc/tgnx_negs.hip; DESIGN §3b-12 has the contract, tests/tgb_negs_ref.py restates it).

TGB ranks each positive of a validation / test split against negatives of which half are destinations the source
interacted with before (and is not interacting with now) and the rest random destinations that are neither; it
generates the lists offline on the CPU and ships them as `*_ns.pkl`.  Here they come from a pair index of the stream:

    idx = PairHistory.build(src, dst, num_nodes)         # each source's distinct destinations + the pair's first row
    idx.contains(src, dst, before=row)                   # bool[n]: the pair occurred at a row < before
    negs = tgb_negatives(src, dst, t, lo, hi, k)         # int64 [hi - lo, k] on the device
    edgebank_mrr(idx, src, dst, negs, lo, hi, batch)     # EdgeBank-inf (pure memorisation) under the same negatives

The draws are counter-based (hash4(seed, tag, event row, draw index)), so a table is a function of its arguments: the
same on every run and for every launch geometry.  Bit parity with TGB's own unseeded numpy draws is not a goal; the
sets (what may be drawn) and the counts are TGB's.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

MAX_K = 1024
_I64_MAX = int(np.iinfo(np.int64).max)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _ids(x, dev) -> torch.Tensor:
    return torch.as_tensor(x).to(dev, torch.long).contiguous()


class PairHistory:
    """CSR of the distinct (source, destination) pairs of rows [0, n) of a stream: indptr int64[N + 1], indices
    int64[nnz] (each source's destinations, ascending), first int64[nnz] (the first row at which the pair occurred).
    `first` lets one index over the whole table answer "seen before row c" for any c."""

    def __init__(self, indptr, indices, first, num_rows: int):
        self.indptr, self.indices, self.first = indptr, indices, first
        self.num_nodes = int(indptr.numel()) - 1
        self.num_rows = int(num_rows)

    @property
    def device(self):
        return self.indptr.device

    @property
    def nnz(self) -> int:
        return int(self.indices.numel())

    @classmethod
    def build(cls, src, dst, num_nodes: int | None = None, device=None) -> "PairHistory":
        dev = _lib.require_device(device if device is not None else (src.device if torch.is_tensor(src) and src.is_cuda
                                                                      else None))
        src, dst = _ids(src, dev), _ids(dst, dev)
        n = int(src.numel())
        if int(dst.numel()) != n:
            raise ValueError("PairHistory.build: src and dst differ in length")
        if num_nodes is None:
            num_nodes = int(torch.maximum(src.max(), dst.max())) + 1 if n else 1
        num_nodes = int(num_nodes)
        if not 0 < num_nodes <= 1 << 32:
            raise ValueError(f"PairHistory.build: num_nodes = {num_nodes} outside [1, 2^32] (ids must be below 2^32)")
        indptr = torch.empty(num_nodes + 1, dtype=torch.long, device=dev)
        indices = torch.empty(max(n, 1), dtype=torch.long, device=dev)
        first = torch.empty(max(n, 1), dtype=torch.long, device=dev)
        nb = _lib.lib().tgnx_pair_index_build_ws_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        nnz = ctypes.c_int64(0)
        _lib.call("tgnx_pair_index_build", _p(src), _p(dst), n, num_nodes, _p(indptr), _p(indices), _p(first),
                  ctypes.byref(nnz), _p(ws), ctypes.c_size_t(nb), _lib.stream(dev))
        return cls(indptr, indices[:nnz.value], first[:nnz.value], n)

    def contains(self, src, dst, before=None) -> torch.Tensor:
        """bool[n]: the pair (src[i], dst[i]) occurred at a row < before (an int for every query, a LongTensor[n] of
        row cuts, or None: anywhere in the indexed rows).  A pair first seen exactly at the cut is not contained."""
        dev = self.device
        src, dst = _ids(src, dev), _ids(dst, dev)
        n = int(src.numel())
        if int(dst.numel()) != n:
            raise ValueError("PairHistory.contains: src and dst differ in length")
        cut, cut_all = None, _I64_MAX
        if torch.is_tensor(before) or isinstance(before, np.ndarray):
            cut = _ids(before, dev)
            if int(cut.numel()) != n:
                raise ValueError("PairHistory.contains: one row cut per query")
        elif before is not None:
            cut_all = int(before)
        out = torch.empty(n, dtype=torch.bool, device=dev)
        _lib.call("tgnx_pair_index_contains", _p(self.indptr), _p(self.indices), _p(self.first), self.num_nodes, _p(src),
                  _p(dst), n, _p(cut), cut_all, _p(out), _lib.stream(dev))
        return out


def hist_rnd(src, dst, t, lo: int, hi: int, k: int, q: int, hist_hi: int, pool, index: PairHistory, seed: int = 0,
             max_draws: int = 0):
    """tgnx_negs_hist_rnd on device tensors, nothing read back: (rows int64 [hi - lo, k], k_hist int32 [hi - lo],
    status int64 [4]).  status = [first output row whose valid set is empty or -1, rows whose historical part was
    filled up, rows whose random part was filled up, rows filled cyclically]."""
    dev = index.device
    lo, hi, k, q = int(lo), int(hi), int(k), int(q)
    n = max(hi - lo, 0)
    out = torch.empty(n, max(k, 0), dtype=torch.long, device=dev)
    k_hist = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.long, device=dev)
    nb = _lib.lib().tgnx_negs_hist_rnd_ws_bytes(index.nnz, n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("tgnx_negs_hist_rnd", _p(src), _p(dst), _p(t), 1 if t.dtype == torch.float64 else 0, int(src.numel()), lo,
              hi, k, q, int(hist_hi), _p(index.indptr), _p(index.indices), _p(index.first), index.num_nodes, index.nnz,
              _p(pool), int(pool.numel()), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(max_draws), _p(out),
              _p(k_hist), _p(status), _p(ws), ctypes.c_size_t(nb), _lib.stream(dev))
    return out, k_hist, status


def tgb_negatives(src, dst, t, lo: int, hi: int, k: int, *, hist_ratio: float = 0.5, hist_hi: int | None = None,
                  pool=None, seed: int = 0, index: PairHistory | None = None, max_draws: int = 0,
                  return_info: bool = False):
    """k `hist_rnd` negatives for every event of rows [lo, hi) of the chronological stream (src, dst, t): int64
    [hi - lo, k] on the device.  Per event, int(k * hist_ratio) (fewer when the source has fewer) destinations its
    source met at rows < hist_hi (default lo: everything before the split) and is not meeting at the event's
    timestamp, ascending; then random destinations of `pool` (sorted unique ids; default unique(dst)) that the source
    neither met before hist_hi nor meets now, ascending.

    t is float64 or float32 and is compared in the type given (float32 merges Unix-second stamps: pass float64).
    index: a PairHistory over the whole table (built here when absent).  Reads the status once (a once-per-split
    call) and raises ValueError naming the row when an event has no valid random destination at all.
    return_info: also (k_hist int32 [hi - lo], status list[4])."""
    dev = _lib.require_device(index.device if index is not None else (src.device if torch.is_tensor(src) and src.is_cuda
                                                                      else None))
    k = int(k)
    if not 0 < k <= MAX_K:
        raise ValueError(f"tgb_negatives: k = {k} outside [1, {MAX_K}]")
    if not 0.0 <= hist_ratio <= 1.0:
        raise ValueError(f"tgb_negatives: hist_ratio = {hist_ratio} outside [0, 1]")
    src, dst = _ids(src, dev), _ids(dst, dev)
    t = torch.as_tensor(t)
    t = t.to(dev, t.dtype if t.dtype in (torch.float64, torch.float32) else torch.float64).contiguous()
    E = int(src.numel())
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= hi <= E) or int(dst.numel()) != E or int(t.numel()) != E:
        raise ValueError(f"tgb_negatives: rows [{lo}, {hi}) outside the {E}-event table, or src / dst / t differ in length")
    if hi - lo > 1 and bool((t[lo + 1:hi] < t[lo:hi - 1]).any()):
        raise ValueError("tgb_negatives: timestamps decrease inside [lo, hi) (the table must be chronological)")
    if index is None:
        index = PairHistory.build(src, dst)
    pool = torch.unique(dst) if pool is None else _ids(pool, dev)
    if int(pool.numel()) == 0:
        raise ValueError("tgb_negatives: empty destination pool")
    q = int(k * hist_ratio)
    out, k_hist, status = hist_rnd(src, dst, t, lo, hi, k, q, lo if hist_hi is None else int(hist_hi), pool, index,
                                   seed=seed, max_draws=max_draws)
    st = status.tolist()                                     # (the one synchronisation)
    if st[0] >= 0:
        raise ValueError(f"tgb_negatives: event row {lo + st[0]} (output row {st[0]}) has no valid random destination: "
                         f"its source has met every destination of the pool")
    return (out, k_hist, st) if return_info else out


def edgebank_mrr(index: PairHistory, src, dst, negs, lo: int, hi: int, batch: int) -> float:
    """MRR of EdgeBank-inf (TGB's memorisation baseline: score 1 for a pair seen before, else 0) over events [lo, hi)
    against negs [hi - lo, K], evaluated in batches of `batch`: a pair counts as seen when it occurred before the
    start row of its batch (the bank is updated after each batch, as the evaluated model's state is).  Ranks are
    tie-averaged as tgnx.data.Evaluator does; the result is the mean over batches of the batch MRR, as test()
    reports it."""
    dev = index.device
    lo, hi, batch = int(lo), int(hi), int(batch)
    negs = torch.as_tensor(negs).to(dev, torch.long)
    n, K = hi - lo, int(negs.shape[1])
    if n <= 0:
        return float("nan")
    s, d = _ids(src, dev)[lo:hi], _ids(dst, dev)[lo:hi]
    rows = torch.arange(lo, hi, device=dev)
    start = lo + (rows - lo) // batch * batch                # start row of each event's batch
    pos = index.contains(s, d, before=start).double()
    neg = index.contains(s.repeat_interleave(K), negs.reshape(-1), before=start.repeat_interleave(K)).view(n, K).double()
    rank = 0.5 * ((neg > pos[:, None]).sum(1) + (neg >= pos[:, None]).sum(1)).double() + 1.0
    rr = (1.0 / rank).cpu().numpy()                          # (exact: ranks are half-integers; the means are numpy's)
    return float(np.mean([rr[a:a + batch].mean() for a in range(0, n, batch)]))
