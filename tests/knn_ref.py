"""numpy restatement of the embedding-space nearest-neighbour operator (tgnx_embed_knn; TgnEngine.similar): float64
dot / cosine scores with the zero-norm rule (a row whose sum of squares is 0 scales by 0: its scores are 0, not NaN),
then the selection and the exclusions of the filtered top-k (tests/topk_filter_ref.py): larger score first, equal
scores (float ==) by lower position, NaN never selected, padding -1 / -inf."""
import numpy as np

from topk_filter_ref import filtered_topk

METRICS = ("dot", "cosine")


def _unit(z):
    """Rows of z (float64) scaled by 1 / sqrt(sum z^2), by 0 where that sum is not > 0 (0 or NaN)."""
    s = (z * z).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(s > 0, 1.0 / np.sqrt(s), 0.0)
    with np.errstate(invalid="ignore"):
        return z * scale[:, None]


def scores(z_q, z_cand, metric):
    """[n_q, n_cand] float64 similarities.  A NaN / inf element makes its row's scores NaN (0 * inf under cosine)."""
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    zq, zc = np.asarray(z_q, dtype=np.float64), np.asarray(z_cand, dtype=np.float64)
    assert zq.ndim == 2 and zc.ndim == 2 and zq.shape[1] == zc.shape[1], (zq.shape, zc.shape)
    if metric == "cosine":
        zq, zc = _unit(zq), _unit(zc)
    with np.errstate(invalid="ignore"):
        return zq @ zc.T


def knn(z_q, z_cand, k, metric="cosine", cand_key=None, q_key=None, excl_ptr=None, excl_key=None):
    """(idx [n_q, k], val [n_q, k] float32, scores [n_q, n_cand] float64): the stable top-k of the reference scores
    (rounded to float32, as the operator compares float32 values) under the key exclusions."""
    s = scores(z_q, z_cand, metric)
    idx, val = filtered_topk(s.astype(np.float32), cand_key, q_key, excl_ptr, excl_key, k)
    return idx, val, s


def select(score_matrix, k, cand_key=None, q_key=None, excl_ptr=None, excl_key=None):
    """The stable filtered top-k of a given float32 score matrix (the operator's own out_all): (idx, val)."""
    return filtered_topk(np.asarray(score_matrix, dtype=np.float32), cand_key, q_key, excl_ptr, excl_key, k)
