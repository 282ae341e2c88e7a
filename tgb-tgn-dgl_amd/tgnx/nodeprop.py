"""TGB node property prediction (the tgbn-* task: NDCG@10) on a link-pretrained, frozen TGN.

Every so often a set of nodes gets a target distribution over C classes; a NodePredictor head (tgnx.nn) on the node
embedding is trained with soft-target cross-entropy and scored with NDCG@k (tgnx.ops.node_loss_ndcg: one pass of the
row kernel gives the loss, its gradient and the metric).  The state side is the engine's: observe_range advances
memory, stores and ring without scoring, embed(nodes) gives the embeddings.  This module adds the label stream and the
loop that interleaves labels with edges:

  LabelStream(t, node, ptr, cls, w, num_classes)   label rows sorted by time, each a sparse target (CSR)
  make_labels(stream, num_classes, period)         labels for a synthetic TemporalStream
  read_node_labels_csv(edge_csv, label_csv)        TGB's <name>_node_labels.csv
  label_schedule(event_t, labels, lo, hi)          which label groups a pass over event rows [lo, hi) predicts, where
  train_node / test_node                           the loops (the TGN paper's protocol for node classification: the
                                                   model stays frozen, only the head's parameters move)

Joint training of memory and attention against the labels is a composition of tgnx.nn.TGNMemory,
GraphAttentionEmbedding and NodePredictor under torch autograd (the head returns dz); the fused engine's train step
has no part in it.
"""
from __future__ import annotations

import csv

import numpy as np
import torch


class LabelStream:
    """Label rows sorted by time; row i is node[i]'s target at time t[i], the sparse vector with weight w[p] at class
    cls[p] for p in [ptr[i], ptr[i + 1]).  The constructor coalesces duplicate (row, class) entries on the host (their
    weights are added; a row's classes come out ascending).  Host arrays: t float64 [R], node int64 [R], ptr int64
    [R + 1], cls int64 [nnz], w float32 [nnz]."""

    def __init__(self, t, node, ptr, cls, w, num_classes: int):
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        node = np.ascontiguousarray(node, dtype=np.int64).reshape(-1)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        cls = np.ascontiguousarray(cls, dtype=np.int64).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        R, C = t.shape[0], int(num_classes)
        if C < 1:
            raise ValueError("LabelStream: num_classes must be positive")
        if node.shape[0] != R or ptr.shape[0] != R + 1:
            raise ValueError("LabelStream: t, node must have R entries and ptr R + 1")
        if ptr[0] != 0 or ptr[-1] != cls.shape[0] or np.any(np.diff(ptr) < 0) or w.shape[0] != cls.shape[0]:
            raise ValueError("LabelStream: ptr must start at 0, not decrease and end at len(cls) = len(w)")
        if R and np.any(np.diff(t) < 0):
            raise ValueError("LabelStream: label rows must be sorted by time")
        if cls.size and (cls.min() < 0 or cls.max() >= C):
            raise ValueError(f"LabelStream: classes must be in [0, {C})")
        if w.size and w.min() < 0:
            raise ValueError("LabelStream: weights must be non-negative")
        row = np.repeat(np.arange(R, dtype=np.int64), np.diff(ptr))
        key, inv = np.unique(row * C + cls, return_inverse=True)           # ascending (row, class), duplicates merged
        self.t, self.node, self.num_classes = t, node, C
        self.cls = key % C
        self.w = np.bincount(inv.reshape(-1), weights=w, minlength=key.shape[0]).astype(np.float32)
        self.ptr = np.zeros(R + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // C, minlength=R), out=self.ptr[1:])
        self._dev = {}

    def __len__(self) -> int:
        return int(self.t.shape[0])

    def groups(self):
        """(T [G] float64, lo [G], hi [G]): the distinct label times in order and each one's row range [lo, hi)."""
        T, lo = np.unique(self.t, return_index=True)
        hi = np.append(lo[1:], len(self)).astype(np.int64)
        return T, lo.astype(np.int64), hi

    def dense(self, lo: int, hi: int, device):
        """y [hi - lo, C] float32 on `device`: the dense targets of rows [lo, hi) (torch plumbing: one index_put)."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= len(self):
            raise ValueError(f"LabelStream.dense: rows [{lo}, {hi}) outside [0, {len(self)})")
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.ptr).to(device), torch.from_numpy(self.cls).to(device),
                              torch.from_numpy(self.w).to(device))
        ptr, cls, w = self._dev[key]
        a, b = int(self.ptr[lo]), int(self.ptr[hi])
        y = torch.zeros(hi - lo, self.num_classes, dtype=torch.float32, device=device)
        if b > a:
            rows = torch.repeat_interleave(torch.arange(hi - lo, device=device), ptr[lo + 1:hi + 1] - ptr[lo:hi],
                                           output_size=b - a)
            y[rows, cls[a:b]] = w[a:b]
        return y


def make_labels(stream, num_classes: int, period: float) -> LabelStream:
    """Labels for a synthetic TemporalStream (tgnx.synth), shaped as TGB's tgbn labels: the class of a destination is
    dst % C; with boundaries T_j = t[0] + j period, node u's target at T_j is the normalised class histogram of u's
    destinations in (T_j, T_{j+1}]; a node without events in that window gets no row.  Rows are ordered by (T_j, u)."""
    C, period = int(num_classes), float(period)
    if period <= 0:
        raise ValueError("make_labels: period must be positive")
    t = np.asarray(stream.t, dtype=np.float64)
    src, dst = np.asarray(stream.src, dtype=np.int64), np.asarray(stream.dst, dtype=np.int64)
    if t.size == 0:
        return LabelStream([], [], [0], [], [], C)
    j = np.ceil((t - t[0]) / period).astype(np.int64) - 1                 # the window (T_j, T_{j+1}] of each event
    ok = j >= 0                                                           # (events at t[0] itself precede T_0's window)
    N = int(max(src.max(), dst.max())) + 1
    rowkey, row = np.unique(j[ok] * N + src[ok], return_inverse=True)     # rows ordered by (j, u)
    row = row.reshape(-1)
    R = rowkey.shape[0]
    cnt = np.bincount(row, minlength=R).astype(np.float64)
    ent, n = np.unique(row * C + dst[ok] % C, return_counts=True)
    ptr = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(ent // C, minlength=R), out=ptr[1:])
    return LabelStream(t[0] + (rowkey // N) * period, rowkey % N, ptr, ent % C, n / cnt[ent // C], C)


def read_node_labels_csv(edge_csv: str, label_csv: str) -> LabelStream:
    """TGB's `<name>_node_labels.csv` — a header line, then `ts, node, class, weight` — for the edge list `edge_csv`
    (`timestamp, source, destination[, ...]`).  PARITY UNPINNED: no TGB file or py-tgb output exists here to check
    the layout against; it restates py-tgb's published convention, as tgnx.tgb_io does.

    Node keys are relabelled exactly as tgb_io.read_edgelist_csv relabels them (0.. in order of first appearance over
    the edge list, source before destination; a labelled node that no edge names is a ValueError), class keys in order
    of first appearance in the label file.  Lines of one (ts, node) form one row; rows are sorted by time (stable).
    The stream also carries `class_keys`, the file's class key of every class id."""
    ids: dict = {}
    with open(edge_csv, newline="") as fh:
        rd = csv.reader(fh)
        next(rd)
        for row in rd:
            if row:
                ids.setdefault(row[1].strip(), len(ids))
                ids.setdefault(row[2].strip(), len(ids))
    classes: dict = {}
    rows: dict = {}
    with open(label_csv, newline="") as fh:
        rd = csv.reader(fh)
        next(rd)
        for line in rd:
            if not line:
                continue
            key = line[1].strip()
            if key not in ids:
                raise ValueError(f"read_node_labels_csv: labelled node {key!r} does not occur in {edge_csv}")
            c = classes.setdefault(line[2].strip(), len(classes))
            rows.setdefault((float(line[0]), ids[key]), []).append((c, float(line[3])))
    keys = list(rows)
    order = np.argsort(np.asarray([k[0] for k in keys], dtype=np.float64), kind="stable")
    t = [keys[i][0] for i in order]
    node = [keys[i][1] for i in order]
    ent = [rows[keys[i]] for i in order]
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in ent])]).astype(np.int64)
    out = LabelStream(t, node, ptr, [c for e in ent for c, _ in e], [w for e in ent for _, w in e],
                      max(len(classes), 1))
    out.class_keys = list(classes)
    return out


def label_schedule(event_t, labels: LabelStream, lo: int, hi: int):
    """The label groups a pass over event rows [lo, hi) predicts, in order, as a list of (r_g, row_lo, row_hi): r_g =
    the number of events with t < T_g (searchsorted left), so group g is predicted after rows [0, r_g) — the edges
    strictly before the label time, TGB's loop — and before an event at the label time itself.  The pass takes the
    groups with lo < r_g <= hi: adjacent passes partition the groups, and a label time before every event (r_g = 0:
    nothing to embed from) belongs to no pass.  The label times are compared in event_t's own format (the engine's
    table holds fp32 times: the labels are rounded to fp32 as the events were)."""
    lo, hi = int(lo), int(hi)
    T, glo, ghi = labels.groups()
    event_t = np.asarray(event_t)
    r = np.searchsorted(event_t, T.astype(event_t.dtype) if event_t.dtype.kind == "f" else T, side="left")
    return [(int(r[g]), int(glo[g]), int(ghi[g])) for g in range(T.shape[0]) if lo < r[g] <= hi]


def _engine(model, neighbor_loader, what):
    from .tgn_epoch import _bound_engine
    eng = _bound_engine(model, neighbor_loader, what)
    if eng.world > 1:
        raise ValueError(f"{what}: one device only (world > 1 is not built)")
    return eng


def _run(eng, neighbor_loader, head, optimizer, labels, lo, hi, batch, k, label_batch, what):
    from . import ops
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= eng.num_events:
        raise ValueError(f"{what}: rows [{lo}, {hi}) outside the event table ({eng.num_events} events)")
    if getattr(eng, "_mode_train", False):                # TGNMemory.train(False), as test() / observe() do
        eng.flush()
        eng._mode_train = False
    sched = label_schedule(eng._tab[2][:eng.num_events].cpu().numpy(), labels, lo, hi)   # the table's fp32 times
    dev = eng.dev
    node = torch.from_numpy(labels.node).to(dev)
    prev, g_loss, g_ndcg, rows_ndcg, n_rows = lo, [], [], [], 0
    for r_g, a, b in sched:
        eng.observe_range(prev, r_g, batch)
        prev = r_g
        z = eng.embed(node[a:b])
        step = (b - a) if not label_batch else int(label_batch)
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        nd_rows = []
        for c in range(a, b, step):
            d = min(b, c + step)
            y = labels.dense(c, d, dev)
            if optimizer is None:
                with torch.no_grad():
                    loss, nd = ops.node_loss_ndcg(head(z[c - a:d - a]), y, k)
            else:
                optimizer.zero_grad(set_to_none=True)
                loss, nd = ops.node_loss_ndcg(head(z[c - a:d - a]), y, k)
                loss.backward()
                optimizer.step()
            loss_sum += loss.detach().double() * (d - c)
            nd_rows.append(nd)
        nd = torch.cat(nd_rows)
        g_loss.append(loss_sum / (b - a))
        g_ndcg.append(nd.mean())
        rows_ndcg.append(nd.sum())
        n_rows += b - a
    eng.observe_range(prev, hi, batch)
    neighbor_loader.cur_e_id = hi
    eng.check()
    G = len(sched)
    if G == 0:
        return {"loss": float("nan"), "ndcg": float("nan"), "ndcg_rows": float("nan"), "groups": 0, "rows": 0,
                "group_ndcg": torch.zeros(0, dtype=torch.float64, device=dev)}
    group_ndcg = torch.stack(g_ndcg)
    stats = torch.stack([torch.stack(g_loss).mean(), group_ndcg.mean(), torch.stack(rows_ndcg).sum() / n_rows]).tolist()
    return {"loss": stats[0], "ndcg": stats[1], "ndcg_rows": stats[2], "groups": G, "rows": n_rows,
            "group_ndcg": group_ndcg}


def train_node(model, neighbor_loader, head, optimizer, labels: LabelStream, lo, hi, batch=None, k=10, reset=True,
               label_batch=None):
    """One pass over event rows [lo, hi) of the engine train() / test() attached to the model that trains `head` (a
    tgnx.nn.NodePredictor on the engine's device) on the label groups the pass meets (label_schedule): per group,
    observe_range(prev, r_g, batch) — memory, stores and ring advance without scoring —, z = embed(group's nodes),
    then head -> node_loss_ndcg -> backward -> optimizer.step() on the head's parameters (in chunks of label_batch
    rows; default the whole group); after the last group the rest of the rows up to hi is observed.  The model stays
    frozen: no parameter of it is read for a gradient or written.  reset: start from reset_state(), as train() does.

    Returns {"loss": mean over groups of the group's mean row loss, "ndcg": mean over groups of the group mean NDCG@k
    (TGB's loop convention), "ndcg_rows": the mean over rows, "groups", "rows", "group_ndcg": float64 [groups] on the
    device}; every metric is of the head as it was when the rows were predicted (before that chunk's step).  Label
    times are compared with the table's fp32 event times in fp32."""
    eng = _engine(model, neighbor_loader, "train_node")
    if reset:
        eng.reset_state()
        eng._mode_train = False
    return _run(eng, neighbor_loader, head, optimizer, labels, lo, hi, batch, k, label_batch, "train_node")


@torch.no_grad()
def test_node(model, neighbor_loader, head, labels: LabelStream, lo, hi, batch=None, k=10, label_batch=None):
    """train_node without the optimizer, continuing from the current stream state: the same observe / embed / head /
    node_loss_ndcg sequence and the same result dict."""
    eng = _engine(model, neighbor_loader, "test_node")
    return _run(eng, neighbor_loader, head, None, labels, lo, hi, batch, k, label_batch, "test_node")


test_node.__test__ = False     # (not a pytest test when re-exported into a test module's namespace)
