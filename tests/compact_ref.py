"""Host restatements for the compaction tests (numpy only; no device, no library): the live set of an event table
from the definition, and what a ring and the message stores name when their event ids are dereferenced.

  ring    nbr / eid [N, K]: slot (v, j) is valid when nbr[v, j] != -1 and then names event eid[v, j];
  stores  nodes [N, 4] = {s_off, s_cnt, d_off, d_cnt} and arena [...]: node v's s run is arena[s_off : s_off + s_cnt],
          its d run arena[d_off : d_off + d_cnt] (the events of the last batch that touched v, in batch order);
  live    row e of the n valid rows is live when a valid ring slot names it, a run holds it, or e >= upto."""
import numpy as np


def store_ids(nodes, arena):
    """(ids, s_cnt, d_cnt): every node's s run then d run, node by node, concatenated."""
    out = []
    for so, sc, do, dc in np.asarray(nodes).tolist():
        out.append(arena[so:so + sc])
        out.append(arena[do:do + dc])
    ids = np.concatenate(out) if out else np.zeros(0, np.int64)
    return ids.astype(np.int64), np.asarray(nodes)[:, 1].copy(), np.asarray(nodes)[:, 3].copy()


def live_rows(nbr, eid, nodes, arena, n, upto=None):
    """Sorted int64 ids of the live rows, and the two reference sets (ring, stores) that make them live."""
    upto = n if upto is None else upto
    ring = set(np.asarray(eid)[np.asarray(nbr) != -1].tolist())
    stores = set(store_ids(nodes, arena)[0].tolist())
    live = ring | stores | set(range(upto, n))
    return np.array(sorted(live), dtype=np.int64), ring, stores


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def deref(h):
    """What the ring and the stores of a host snapshot h (keys nbr, eid, rt, nodes, arena, src, dst, t, msg) name:
    a dict of arrays that must be bit-identical before and after a renumbering."""
    valid = h["nbr"] != -1
    out = dict(nbr=h["nbr"], valid=valid, rt=_bits(np.where(valid, h["rt"], np.float32(0))))
    ids, sc, dc = store_ids(h["nodes"], h["arena"])
    out["s_cnt"], out["d_cnt"] = sc, dc
    e = h["eid"][valid]
    for k in ("src", "dst", "t", "msg"):
        out["ring_" + k] = _bits(h[k][e])
        out["store_" + k] = _bits(h[k][ids])
    return out


def assert_same_deref(a, b):
    da, db = deref(a), deref(b)
    for k in da:
        assert np.array_equal(da[k], db[k]), k
