"""GPU checks of the embedding-space nearest-neighbour operator (csrc/tgnx_knn.hip; torch.ops.tgnx.embed_knn,
tgnx.ops.embed_knn): all-pairs dot / cosine scores on the f32 MFMA with the top-k selection fused in.

The reference is tests/knn_ref.py: float64 scores with the zero-norm rule, the filtered top-k's selection.  Per case
and metric, in the manner of test_gpu_link_topk.py:
  * the returned scores match it at 2e-5 in the project's `_close` metric (max |a - b| over max(|b|, 1): the
    tolerance the predictor operators are held to; the f32 MFMA chain's error is bounded by about 1.5e-7 · Σ|a·b|
    at K <= 1024, far inside it at these shapes);
  * (idx, val) equal EXACTLY the stable top-k of the returned scores row, padding idx -1 / val -inf;
  * against the reference without assuming equal rounding: with tol = 2e-5 and scale = max(|ref|, 1), every selected
    candidate's reference score is >= the reference's k-th largest - 2 tol scale, the returned values match the
    reference at the returned positions within tol scale, and the k candidates are distinct (every case, no cap);
  * grid independence, bit for bit: a rerun with a permuted subset of the queries and the candidates in another
    order at another n_cand (another chunk count; at 10,000 candidates the other chunk width too) gives the same
    pairs the same int32 bit patterns;
  * exclusions (cand_key with a duplicated node, q_key, exclude segments by q mod 4: none / a few keys at chunk
    edges and keys matching nothing / every candidate / all but fewer than k) equal knn_ref's selection on the
    returned scores, the scores themselves are unmasked, and a query without exclusions gets the unfiltered result.
Shapes (n_q, n_cand, D, k): one pair; fewer candidates than k; a partial query tile, a partial chunk and a partial
16-candidate sub-tile; D no multiple of 4; D = 3 (a row shorter than one 16-byte vector); D = 256 and k = 128 over 12
chunks; 200 x 10,000 (13 tiles x 20 chunks of 512).  One case with a NaN row and a zero row among the candidates and
a zero query; one call captured in a graph and replayed twice."""
import numpy as np
import pytest
import torch

import knn_ref
from test_gpu_topk_filter import _exclusions

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 2e-5

#        n_q, n_cand, D, k
CASES = [(1, 1, 100, 1), (3, 5, 100, 10), (17, 257, 100, 10), (70, 600, 30, 5), (3, 300, 3, 2), (5, 3000, 256, 128),
         (200, 10000, 100, 10)]
PARAMS = [(c, m) for c in CASES for m in knn_ref.METRICS]
IDS = ["x".join(map(str, c)) + "-" + m for c, m in PARAMS]


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long).to(DEV)


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1.0) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _stable_topk(row: np.ndarray, k: int):
    """(positions, values) of the k largest entries, equal values by lower position; -1 / -inf padding."""
    order = np.lexsort((np.arange(row.size), -row))[:k]
    idx = np.full(k, -1, dtype=np.int64)
    val = np.full(k, -np.inf, dtype=np.float32)
    idx[:order.size] = order
    val[:order.size] = row[order]
    return idx, val


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def cases():
    """Every (case, metric)'s operands, float64 reference scores and the operator's three outputs, computed once
    and left unchanged."""
    from tgnx import ops
    out = {}
    for c in CASES:
        n_q, n_cand, D, k = c
        torch.manual_seed(n_q + n_cand + D)
        zq, zc = torch.randn(n_q, D), torch.randn(n_cand, D)
        for m in knn_ref.METRICS:
            got = ops.embed_knn(zq.to(DEV), zc.to(DEV), k, metric=m, return_scores=True)
            out[(c, m)] = dict(zq=zq, zc=zc, ref=knn_ref.scores(zq.numpy(), zc.numpy(), m),
                               got=tuple(t.cpu() for t in got), dev=got)
    return out


@pytest.mark.parametrize("case,metric", PARAMS, ids=IDS)
def test_scores_match_the_float64_reference(cases, case, metric):
    c = cases[(case, metric)]
    assert tuple(c["got"][2].shape) == c["ref"].shape
    _close(c["got"][2].numpy(), c["ref"], TOL)


@pytest.mark.parametrize("case,metric", PARAMS, ids=IDS)
def test_selection_is_the_stable_topk_of_the_returned_scores(cases, case, metric):
    val, idx, scores = (t.numpy() for t in cases[(case, metric)]["got"])
    k = case[3]
    assert val.shape == idx.shape == (scores.shape[0], k)
    for q in range(scores.shape[0]):
        wi, wv = _stable_topk(scores[q], k)
        assert np.array_equal(idx[q], wi), (q, idx[q], wi)
        assert np.array_equal(val[q], wv), (q, val[q], wv)


@pytest.mark.parametrize("case,metric", PARAMS, ids=IDS)
def test_selection_against_the_reference(cases, case, metric):
    c = cases[(case, metric)]
    n_q, n_cand, _, k = case
    ref = c["ref"]
    val, idx = c["got"][0].double().numpy(), c["got"][1].numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    kk = min(k, n_cand)
    assert (idx[:, :kk] >= 0).all() and (idx[:, :kk] < n_cand).all() and (idx[:, kk:] == -1).all()
    assert np.isneginf(val[:, kk:]).all()
    for q in range(n_q):
        assert len(set(idx[q, :kk].tolist())) == kk                     # k distinct candidates
        kth = np.sort(ref[q])[::-1][kk - 1]
        at = ref[q, idx[q, :kk]]
        assert (at >= kth - 2 * TOL * scale).all(), (q, float((kth - at).max()), 2 * TOL * scale)
        assert np.abs(val[q, :kk] - at).max() <= TOL * scale


@pytest.mark.parametrize("case,metric", PARAMS, ids=IDS)
def test_a_pairs_bits_do_not_depend_on_the_grid(cases, case, metric):
    """A permuted subset of the queries against two thirds of the candidates in another order: other tiles, other
    sub-tiles, another chunk count (200 x 10,000 -> 6,666: 256-candidate chunks instead of 512)."""
    from tgnx import ops
    c = cases[(case, metric)]
    n_q, n_cand, _, k = case
    rng = np.random.default_rng(n_q * 7 + n_cand)
    qp = rng.permutation(n_q)[:max(1, (2 * n_q + 2) // 3)]
    cp = rng.permutation(n_cand)[:max(1, (2 * n_cand) // 3)]
    zq, zc = c["zq"][torch.from_numpy(qp)].to(DEV), c["zc"][torch.from_numpy(cp)].to(DEV)
    val, idx, scores = ops.embed_knn(zq, zc, min(k, 7), metric=metric, return_scores=True)
    want = c["got"][2][torch.from_numpy(qp)][:, torch.from_numpy(cp)]
    assert torch.equal(_bits(scores.cpu()), _bits(want))
    # and the selection of the rerun is consistent with its own scores
    s = scores.cpu().numpy()
    for q in range(0, len(qp), max(1, len(qp) // 5)):
        wi, wv = _stable_topk(s[q], min(k, 7))
        assert np.array_equal(idx[q].cpu().numpy(), wi) and np.array_equal(val[q].cpu().numpy(), wv)


@pytest.mark.parametrize("case,metric", PARAMS, ids=IDS)
def test_exclusions_by_key(cases, case, metric):
    from tgnx import ops
    c = cases[(case, metric)]
    n_q, n_cand, _, k = case
    rng = np.random.default_rng(n_q + n_cand)
    key = rng.permutation(4 * n_cand)[:n_cand].astype(np.int64) + 50
    if n_cand > 1:
        key[n_cand - 1] = key[1]                                  # one node at two positions
    qkey = np.where(rng.random(n_q) < 0.7, key[rng.integers(0, n_cand, n_q)], -1).astype(np.int64)
    qkey[::8] = -1                                                # with q mod 4 == 0: queries without any exclusion
    eptr, ekey = _exclusions(rng, n_q, n_cand, k, key)
    zq, zc = c["zq"].to(DEV), c["zc"].to(DEV)
    val, idx, scores = ops.embed_knn(zq, zc, k, metric=metric, return_scores=True, cand_key=_dev(key),
                                     q_key=_dev(qkey), exclude=(_dev(eptr), _dev(ekey)))
    assert torch.equal(_bits(scores.cpu()), _bits(c["got"][2]))             # unmasked, and the same bits
    wi, wv = knn_ref.select(scores.cpu().numpy(), k, key, qkey, eptr, ekey)
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(val.cpu().numpy(), wv)
    free = [q for q in range(n_q) if qkey[q] == -1 and eptr[q] == eptr[q + 1]]
    assert n_q == 1 or free
    for q in free:                                                # no exclusion: exactly the unfiltered result
        assert torch.equal(idx[q].cpu(), c["got"][1][q]) and torch.equal(val[q].cpu(), c["got"][0][q])
    # the single rules on their own: positions as keys with q_key, and cand_key alone (nothing excluded)
    own = np.minimum(np.arange(n_q), n_cand - 1).astype(np.int64)
    v2, i2 = ops.embed_knn(zq, zc, k, metric=metric, q_key=_dev(own))
    wi, wv = knn_ref.select(c["got"][2].numpy(), k, None, own, None, None)
    assert np.array_equal(i2.cpu().numpy(), wi) and np.array_equal(v2.cpu().numpy(), wv)
    v3, i3 = ops.embed_knn(zq, zc, k, metric=metric, cand_key=_dev(key))
    assert torch.equal(i3.cpu(), c["got"][1]) and torch.equal(v3.cpu(), c["got"][0])


@pytest.mark.parametrize("metric", knn_ref.METRICS)
def test_a_nan_row_and_a_zero_row(metric):
    from tgnx import ops
    torch.manual_seed(21)
    n_q, n_cand, D, k = 6, 40, 100, 40
    zq, zc = torch.randn(n_q, D), torch.randn(n_cand, D)
    zc[7, 13] = float("nan")
    zc[19] = 0.0
    zq[4] = 0.0
    val, idx, scores = (t.cpu().numpy() for t in ops.embed_knn(zq.to(DEV), zc.to(DEV), k, metric=metric,
                                                               return_scores=True))
    ref = knn_ref.scores(zq.numpy(), zc.numpy(), metric)
    assert np.isnan(scores[:, 7]).all() and np.isnan(ref[:, 7]).all()
    ok = np.ones(n_cand, dtype=bool)
    ok[7] = False
    assert not np.isnan(scores[:, ok]).any()
    assert (scores[:, 19] == 0).all() and (scores[4, ok] == 0).all()        # the zero rows: 0, not NaN
    _close(scores[:, ok], ref[:, ok], TOL)
    assert (idx != 7).all() and (idx[:, -1] == -1).all() and np.isneginf(val[:, -1]).all()
    assert (idx[:, :-1] >= 0).all()
    assert np.array_equal(idx[4, :-1], np.flatnonzero(ok))                 # all ties: by position, the NaN skipped
    wi, wv = knn_ref.select(scores, k)
    assert np.array_equal(idx, wi) and np.array_equal(val, wv)


def test_no_queries_and_no_candidates():
    from tgnx import ops
    z = torch.randn(5, 32, device=DEV)
    val, idx, scores = ops.embed_knn(z, torch.zeros(0, 32, device=DEV), 3, return_scores=True)
    assert scores.shape == (5, 0)
    assert bool((idx == -1).all()) and bool(torch.isinf(val).all()) and bool((val < 0).all())
    val, idx = ops.embed_knn(torch.zeros(0, 32, device=DEV), z, 3, metric="dot")
    assert val.shape == (0, 3) and idx.shape == (0, 3)


def test_repeat_call_and_graph_replay_give_the_same_result():
    from tgnx import ops
    torch.manual_seed(2)
    zq, zc = torch.randn(70, 100, device=DEV), torch.randn(600, 100, device=DEV)
    own = torch.arange(70, device=DEV)
    first = ops.embed_knn(zq, zc, 10, return_scores=True, q_key=own)
    again = ops.embed_knn(zq, zc, 10, return_scores=True, q_key=own)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops.embed_knn(zq, zc, 10, return_scores=True, q_key=own)
    for _ in range(2):
        for t in cap:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(first, cap):
            assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
