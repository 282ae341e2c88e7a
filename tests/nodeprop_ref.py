"""numpy float64 restatement of node property prediction (csrc/tgnx_nodeprop.hip; tgnx.ops.node_predictor,
soft_cross_entropy, ndcg_at_k): NodePredictor's forward and backward (modules/decoder.py:30-41), the soft-target
cross-entropy with its gradient, and NDCG@k as sklearn's ndcg_score defines it with its default tie handling:

    gt_c = classes scoring above c, eq_c = classes scoring equal to c (c included)
    disc[r] = 1 / log2(r + 1) for ranks r = 1..min(k, C), 0 beyond; cum[j] = the sum of the first j discounts
    DCG  = Σ_c y_c (cum[gt_c + eq_c] − cum[gt_c]) / eq_c      (tied scores share the mean discount of their ranks)
    IDCG = Σ_{r <= k} (the r-th largest y) disc[r];  ndcg = DCG / IDCG, 0 where IDCG = 0

Scores are compared as given (the GPU tests pass the operator's own float32 logits)."""
import numpy as np


def head_forward(z, w1, b1, w2, b2):
    """(logits [M, C], h [M, D]) = (relu(z W1^T + b1) W2^T + b2, relu(z W1^T + b1)) in float64."""
    z, w1, b1, w2, b2 = (np.asarray(a, dtype=np.float64) for a in (z, w1, b1, w2, b2))
    h = np.maximum(z @ w1.T + b1, 0.0)
    return h @ w2.T + b2, h


def head_backward(dlogits, z, h, w1, w2):
    """The gradients of head_forward given dlogits: dict(dz, dw1, db1, dw2, db2)."""
    g, z, h, w1, w2 = (np.asarray(a, dtype=np.float64) for a in (dlogits, z, h, w1, w2))
    dh = (g @ w2) * (h > 0)
    return dict(dw2=g.T @ h, db2=g.sum(0), dw1=dh.T @ z, db1=dh.sum(0), dz=dh @ w1)


def soft_ce(logits, y, scale=None):
    """(loss_rows [M], dlogits [M, C]): loss_i = lse_i Σ_c y_ic − Σ_c y_ic l_ic and dlogits = (softmax(l_i) Σ_c y_ic −
    y_i) scale (default 1 / M: the gradient of the mean loss).  The targets need not sum to 1."""
    l, y = np.asarray(logits, dtype=np.float64), np.asarray(y, dtype=np.float64)
    M = l.shape[0]
    mx = l.max(axis=1, keepdims=True) if l.size else np.zeros((M, 1))
    e = np.exp(l - mx)
    se = e.sum(axis=1, keepdims=True)
    lse = mx + np.log(se)
    sy = y.sum(axis=1, keepdims=True)
    loss = (lse * sy).reshape(-1) - (y * l).sum(axis=1)
    scale = (1.0 / M if M else 0.0) if scale is None else scale
    return loss, (e / se * sy - y) * scale


def ndcg_cum(k):
    cum = np.zeros(k + 1)
    cum[1:] = np.cumsum(1.0 / np.log2(np.arange(1, k + 1) + 1.0))
    return cum


def ndcg_rows(logits, y, k=10):
    """float64 [M]: NDCG@k of every row under the definition above."""
    l, y = np.asarray(logits), np.asarray(y, dtype=np.float64)
    M, C = l.shape
    kk = min(k, C)
    cum = np.concatenate([ndcg_cum(kk), np.full(C + 1, ndcg_cum(kk)[-1])])   # cum[j] for every j up to C (+ slack)
    disc = np.diff(cum)[:C]
    out = np.zeros(M)
    for i in range(M):
        pos = np.nonzero(y[i] > 0)[0]
        idcg = float((np.sort(y[i])[::-1][:kk] * disc[:kk]).sum())
        if idcg <= 0:
            continue
        dcg = 0.0
        for c in pos:
            gt = int((l[i] > l[i, c]).sum())
            eq = int((l[i] == l[i, c]).sum())
            dcg += y[i, c] * (cum[gt + eq] - cum[gt]) / eq
        out[i] = dcg / idcg
    return out
