"""Numpy restatement of tgnx_link_predictor_rank's counting rule (include/tgnx.h), on a given logit matrix.

For source q with target position p = target[q] and key(c) = cand_key[c] (default: c), the compared set S_q is every
position c in [0, n_count) with c != p, key(c) != key(p) (only when p lies inside the matrix), key(c) != src_key[q],
key(c) not in excl_key[excl_ptr[q] : excl_ptr[q + 1]], and logits[q, c] not NaN.  gt / eq count the members of S_q
whose logit is above / equal to (float ==) tl = logits[q, p]; n = |S_q|; rank = 1 + gt + eq / 2.  A skipped row (p
outside [0, n_cand) or tl NaN) has gt = eq = 0, rank NaN and n as defined."""
import numpy as np


def link_rank_ref(logits, n_count, target, cand_key=None, src_key=None, excl_ptr=None, excl_key=None):
    logits = np.asarray(logits)
    n_src, n_cand = logits.shape
    key = np.arange(n_cand, dtype=np.int64) if cand_key is None else np.asarray(cand_key, dtype=np.int64)
    gt, eq, n = (np.zeros(n_src, dtype=np.int64) for _ in range(3))
    rank = np.full(n_src, np.nan, dtype=np.float64)
    pos = np.arange(n_count)
    for q in range(n_src):
        p = int(target[q])
        inside = 0 <= p < n_cand
        row = logits[q, :n_count]
        ok = ~np.isnan(row)
        if inside:
            ok &= (pos != p) & (key[:n_count] != key[p])
        if src_key is not None:
            ok &= key[:n_count] != int(src_key[q])
        if excl_ptr is not None:
            ok &= ~np.isin(key[:n_count], np.asarray(excl_key)[int(excl_ptr[q]):int(excl_ptr[q + 1])])
        n[q] = int(ok.sum())
        if not inside or np.isnan(logits[q, p]):
            continue
        tl = logits[q, p]
        gt[q] = int((row[ok] > tl).sum())
        eq[q] = int((row[ok] == tl).sum())
        rank[q] = 1.0 + gt[q] + 0.5 * eq[q]
    return gt, eq, n, rank
