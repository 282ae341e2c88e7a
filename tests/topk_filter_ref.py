"""numpy restatement of the filtered / per-source-list top-k selection (tgnx_link_predictor_topk_filtered,
tgnx_link_predictor_topk_lists; TgnEngine.recommend_filtered).  The order is the operators': larger logit first, equal
logits (float ==) by lower position / slot, NaN never selected, padding -1 / -inf."""
import numpy as np


def _stable(row, allowed, k):
    """(positions, values) of the k largest allowed, non-NaN entries of row; equal values by lower position."""
    pos = np.flatnonzero(allowed & ~np.isnan(row))
    order = pos[np.lexsort((pos, -row[pos]))][:k]
    idx = np.full(k, -1, dtype=np.int64)
    val = np.full(k, -np.inf, dtype=np.float32)
    idx[:order.size] = order
    val[:order.size] = row[order]
    return idx, val


def filtered_topk(logits, cand_key, src_key, excl_ptr, excl_key, k):
    """Stable top-k of every row of logits [n_src, n_cand] after removing, for row q, the candidates whose key
    (cand_key[c]; None: c) equals src_key[q] (None: no such rule) or occurs in excl_key[excl_ptr[q]:excl_ptr[q+1]]
    (excl_ptr None: no lists).  Returns (idx [n_src, k], val [n_src, k])."""
    logits = np.asarray(logits, dtype=np.float32)
    n_src, n_cand = logits.shape
    key = np.arange(n_cand, dtype=np.int64) if cand_key is None else np.asarray(cand_key, dtype=np.int64)
    idx = np.full((n_src, k), -1, dtype=np.int64)
    val = np.full((n_src, k), -np.inf, dtype=np.float32)
    for q in range(n_src):
        allowed = np.ones(n_cand, dtype=bool)
        if src_key is not None:
            allowed &= key != int(src_key[q])
        if excl_ptr is not None:
            allowed &= ~np.isin(key, np.asarray(excl_key[int(excl_ptr[q]):int(excl_ptr[q + 1])], dtype=np.int64))
        idx[q], val[q] = _stable(logits[q], allowed, k)
    return idx, val


def lists_topk(ragged_logits, ptr, k):
    """Stable top-k inside every segment of ragged_logits [nnz] (NaN: a skipped entry): (slot [n_src, k] offsets
    inside the segment, val [n_src, k])."""
    lg = np.asarray(ragged_logits, dtype=np.float32)
    n_src = len(ptr) - 1
    slot = np.full((n_src, k), -1, dtype=np.int64)
    val = np.full((n_src, k), -np.inf, dtype=np.float32)
    for q in range(n_src):
        row = lg[int(ptr[q]):int(ptr[q + 1])]
        slot[q], val[q] = _stable(row, np.ones(row.size, dtype=bool), k)
    return slot, val


def seen_lists(neighbors, e_id, src):
    """(ptr, keys): for every source the ascending node ids of its neighbour-ring row, an entry counting only where
    e_id >= 0 (a reset ring keeps stale ids in `neighbors`)."""
    neighbors, e_id = np.asarray(neighbors), np.asarray(e_id)
    rows = [np.sort(neighbors[s][e_id[s] >= 0]).astype(np.int64) for s in np.asarray(src).reshape(-1)]
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([r.size for r in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64))
