"""GPU checks of the link-rank operator (csrc/tgnx_topk.hip: rank_target, rank_pairs; torch.ops.tgnx.predictor_rank,
tgnx.ops.link_rank).

The operator is held to the dense top-k operator bit for bit and to tests/link_rank_ref.py exactly: tlogit[q] is
torch.equal to ops.link_topk(return_scores=True)'s logits at [q, target[q]], and (gt, eq, n) equal the numpy
restatement on those logits.  Against the oracle (RefLinkPredictor over all pairs on the CPU) without assuming equal
rounding: with tol = 2e-5, scale = max(|ref|, 1) and r the reference logits over the compared set,
#{r > r_t + 2 tol scale} <= gt and gt + eq <= #{r >= r_t - 2 tol scale}.  So that this is not vacuous the two bounds
coincide on the reference alone for at least 9 in 10 rows that are neither tied on purpose nor skipped; the shares
observed on the CPU with the seeds below: 1x1 1/1, 17x257 12/12, 70x600 58/59, 5x3000 3/3, 3x300 2/2 (asserted again
here).

Shapes (n_src, n_cand, d_in, D), from test_gpu_topk_filter.py: the smallest; two source tiles, one partial, and a
chunk boundary (the chunk is 256); D no multiple of 4; many chunks and an exclusion list of 3,000 keys (past the
1,024-key LDS staging); D = 3, a row of one 16-byte vector, shorter than the pair loop's load group (the seed is one
at which the +inf entry meets weights of both signs, so that its column is NaN at D = 3 as well).  Every shape runs with n_count = n_cand and with n_count = n_cand - 3 (targets in rows past
n_count).  Targets, by source: 0, 255 (the last position of a chunk), 256 (the first of the next), -1 (skipped),
n_cand - 1, n_cand (skipped), n_cand - 2, n_cand - 4, then random.  Sources q = 0 mod 8 (no exclusions) get two exact
copies of their target's z_cand row: one under another key (it must land in eq), one under the target's key (in no
count).  Exclusions by q mod 4 as test_gpu_topk_filter._exclusions builds them: none; keys at chunk edges, duplicates
and keys matching nothing; every key (n = 0, rank 1; the list names the target's own key, which changes nothing); all
but a few.  cand_key carries one node at two positions; src_key names a candidate's node for most sources.

NaN: position 6 of z_cand holds one +inf entry, which makes every logit of that column NaN (+inf and -inf meet in the
contraction) in the dense operator and in the oracle alike: it is in no count.  Position 5 is a row of NaN: the
chain's ReLU is a max that returns its non-NaN operand, so the dense operator scores that row as b_out, not NaN; the
rank operator must treat it exactly as those logits say (the exactness check), whatever they are."""
import numpy as np
import pytest
import torch

from link_rank_ref import link_rank_ref
from test_gpu_topk_filter import LCHUNK, _args, _dev, _exclusions, _ref_logits, _weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 2e-5
K = 10
NANPOS, INFPOS = 5, 6

#        n_src, n_cand, d_in, D
CASES = [(1, 1, 100, 100), (17, 257, 100, 100), (70, 600, 30, 30), (5, 3000, 32, 32), (3, 300, 5, 3)]
IDS = ["x".join(map(str, c)) for c in CASES]
SEEDS = {CASES[0]: 2, CASES[1]: 274, CASES[2]: 670, CASES[3]: 3005, CASES[4]: 313}


def _inputs(case):
    """CPU side of a case: weights, z rows (clean: before the NaN / inf rows go in), targets, keys, exclusions."""
    n_src, n_cand, d_in, D = case
    seed = SEEDS[case]
    rng = np.random.default_rng(seed)
    lins = _weights(d_in, D, seed=seed)
    zs, zc = torch.randn(n_src, d_in), torch.randn(n_cand, d_in)
    key = rng.permutation(4 * n_cand)[:n_cand].astype(np.int64) + 50
    big = n_cand > 16
    if big:
        key[n_cand - 1] = key[1]                                  # one node at two positions
        fixed = [0, LCHUNK - 1, LCHUNK, -1, n_cand - 1, n_cand, n_cand - 2, n_cand - 4]
        free = np.setdiff1d(np.arange(30, n_cand - 5), [LCHUNK - 1, LCHUNK])
        # past the fixed ones: random targets, and for q = 1 mod 4 the candidate the oracle ranks first (a rank near 1)
        ref0 = _ref_logits(lins, zs, zc).numpy()
        target = np.array([fixed[q] if q < 8 else int(free[np.argmax(ref0[q, free])]) if q % 4 == 1 else
                           int(rng.choice(free)) for q in range(n_src)], dtype=np.int64)
    else:
        target = np.zeros(n_src, dtype=np.int64)
    tied, same_key = {}, {}
    if big:
        for i, q in enumerate(range(0, n_src, 8)):                # two copies of the target's row at positions 10 ..
            a, b = 10 + 2 * i, 11 + 2 * i
            zc[a] = zc[target[q]]
            zc[b] = zc[target[q]]
            key[b] = key[target[q]]
            tied[q], same_key[q] = a, b
    skey = np.where(rng.random(n_src) < 0.7, key[rng.integers(0, n_cand, n_src)], -1).astype(np.int64)
    skey[::8] = -1                                                # with q mod 4 == 0: sources without any exclusion
    eptr, ekey = _exclusions(rng, n_src, n_cand, K, key)
    zc_clean = zc.clone()
    if big:
        zc[NANPOS] = float("nan")
        zc[INFPOS, 0] = float("inf")
    return dict(lins=lins, zs=zs, zc=zc, zc_clean=zc_clean, key=key, skey=skey, eptr=eptr, ekey=ekey, target=target,
                tied=tied, same_key=same_key, big=big)


def _compared(c, q, n_count):
    """The compared set of source q by the key rules alone (no NaN rule)."""
    key, p = c["key"], int(c["target"][q])
    ok = np.ones(n_count, dtype=bool)
    if 0 <= p < key.size:
        ok &= (np.arange(n_count) != p) & (key[:n_count] != key[p])
    ok &= key[:n_count] != c["skey"][q]
    return ok & ~np.isin(key[:n_count], c["ekey"][c["eptr"][q]:c["eptr"][q + 1]])


def _bracket(c, ref, n_count, rows):
    """Per row of `rows`: (#{r > r_t + 2 tol scale}, #{r >= r_t - 2 tol scale}) on the reference logits."""
    ref = np.asarray(ref, dtype=np.float64)
    m = 2 * TOL * max(float(np.nanmax(np.abs(ref))), 1.0)
    out = {}
    for q in rows:
        r = ref[q, :n_count][_compared(c, q, n_count)]
        r = r[~np.isnan(r)]
        rt = ref[q, c["target"][q]]
        out[q] = (int((r > rt + m).sum()), int((r >= rt - m).sum()))
    return out


def _ranked_rows(c, n_cand):
    return [q for q in range(len(c["target"])) if 0 <= c["target"][q] < n_cand]


def _kw(c):
    return dict(cand_key=_dev(c["key"]), src_key=_dev(c["skey"]), exclude=(_dev(c["eptr"]), _dev(c["ekey"])))


@pytest.fixture(scope="module")
def cases():
    """Every case's inputs, the dense operator's logits and the rank operator's outputs, computed once and left
    unchanged."""
    from tgnx import ops
    out = {}
    for case in CASES:
        n_src, n_cand, d_in, D = case
        c = _inputs(case)
        a = _args(c["lins"])
        zs, zc, zcc = c["zs"].to(DEV), c["zc"].to(DEV), c["zc_clean"].to(DEV)
        c["args"] = a
        c["dense"] = ops.link_topk(zs, zc, *a, 1, sigmoid=False, return_scores=True)[2]
        c["counts"] = (n_cand, max(n_cand - 3, 0))
        c["rank"] = {nc: ops.link_rank(zs, zc, *a, _dev(c["target"]), n_count=nc, **_kw(c)) for nc in c["counts"]}
        c["rank_clean"] = ops.link_rank(zs, zcc, *a, _dev(c["target"]), **_kw(c))
        c["topk"] = ops.link_topk(zs, zc, *a, K, sigmoid=False, **_kw(c))
        out[case] = c
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_target_logit_has_the_dense_operators_bits(cases, case):
    c = cases[case]
    n_cand = case[1]
    dense = c["dense"].cpu()
    for nc in c["counts"]:
        tl = c["rank"][nc][4].cpu()
        for q, p in enumerate(c["target"]):
            if 0 <= p < n_cand:
                assert tl[q].view(torch.int32) == dense[q, p].view(torch.int32), (nc, q, p)
            else:
                assert bool(torch.isnan(tl[q])), (nc, q, p)
    rows = _ranked_rows(c, n_cand)
    rows = torch.as_tensor(rows)
    assert torch.equal(c["rank"][n_cand][4].cpu()[rows], dense[rows, torch.as_tensor(c["target"])[rows]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_are_the_reference_on_those_logits(cases, case):
    c = cases[case]
    n_src, n_cand = case[:2]
    dense = c["dense"].cpu().numpy()
    for nc in c["counts"]:
        rank, gt, eq, n, tl = (t.cpu().numpy() for t in c["rank"][nc])
        wgt, weq, wn, wrank = link_rank_ref(dense, nc, c["target"], c["key"], c["skey"], c["eptr"], c["ekey"])
        print(f"n_count {nc}: gt {gt[:8]} eq {eq[:8]} n {n[:8]}")
        assert np.array_equal(n, wn), (nc, np.flatnonzero(n != wn)[:5], n[:8], wn[:8])
        assert np.array_equal(gt, wgt), (nc, np.flatnonzero(gt != wgt)[:5])
        assert np.array_equal(eq, weq), (nc, np.flatnonzero(eq != weq)[:5])
        assert np.array_equal(rank, wrank, equal_nan=True)
        assert rank.dtype == np.float64 and gt.dtype == eq.dtype == n.dtype == np.int64 and tl.dtype == np.float32
        for q, p in enumerate(c["target"]):
            if not 0 <= p < n_cand:                               # skipped: no counts, NaN rank, n as defined
                assert gt[q] == 0 and eq[q] == 0 and np.isnan(rank[q]) and np.isnan(tl[q])
                assert n[q] == (_compared(c, q, nc) & ~np.isnan(dense[q, :nc])).sum()
        for q in range(n_src):
            if q % 4 == 2 or n_src == 1:                          # every key listed, the target's own among them
                assert n[q] == 0 and gt[q] == 0 and eq[q] == 0
                assert rank[q] == 1.0 or not 0 <= c["target"][q] < n_cand
    if c["big"]:
        assert c["target"][2] == LCHUNK and c["rank"][n_cand][0][2] == 1.0 and not np.isnan(c["rank"][n_cand][4][2].item())
        if n_src > 4:                                             # a target past n_count is ranked against all n_count
            assert c["target"][4] == n_cand - 1 and c["rank"][n_cand - 3][3][4] > 0


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_forced_ties_and_nan_logits(cases, case):
    c = cases[case]
    n_src, n_cand = case[:2]
    dense = c["dense"].cpu().numpy()
    assert np.isnan(dense[:, INFPOS]).all()                       # the premise: that column's logits are NaN
    print("logits of the NaN row:", dense[:3, NANPOS], "b_out", float(c["args"][5]))
    for nc in c["counts"]:
        rank, gt, eq, n, tl = (t.cpu().numpy() for t in c["rank"][nc])
        for q, a in c["tied"].items():
            b, p = c["same_key"][q], c["target"][q]
            assert dense[q, a] == dense[q, p] == dense[q, b]
            assert eq[q] >= 1, (nc, q)
            # without the two copies: the same gt, one tie fewer, one compared fewer (the same-key copy never counted)
            keep = np.ones(n_cand, dtype=bool)
            keep[[a, b]] = False
            pos = np.cumsum(keep) - 1
            wgt, weq, wn, _ = link_rank_ref(dense[q:q + 1, keep], int(keep[:nc].sum()), [pos[p]], c["key"][keep])
            assert (gt[q], eq[q] - 1, n[q] - 1) == (wgt[0], weq[0], wn[0]), (nc, q)
        # the NaN column is in no count: with it cut out of the logits, every count is the same
        keep = np.ones(n_cand, dtype=bool)
        keep[INFPOS] = False
        pos = np.cumsum(keep) - 1
        t2 = np.where((c["target"] >= 0) & (c["target"] < n_cand), pos[np.clip(c["target"], 0, n_cand - 1)],
                      np.where(c["target"] < 0, -1, n_cand - 1))
        wgt, weq, wn, _ = link_rank_ref(dense[:, keep], nc - 1, t2, c["key"][keep], c["skey"], c["eptr"], c["ekey"])
        assert np.array_equal(gt, wgt) and np.array_equal(eq, weq) and np.array_equal(n, wn), nc
    free = [q for q in range(n_src) if q % 8 == 0]                # no exclusions at all: everything else competes
    n = c["rank"][n_cand][3].cpu().numpy()
    for q in free:
        dup = int((c["key"] == c["key"][c["target"][q]]).sum())
        assert n[q] == n_cand - dup - int(np.isnan(dense[q]).sum()), q


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_src_key_removes_the_sources_node(cases, case):
    from tgnx import ops
    c = cases[case]
    n_src, n_cand = case[:2]
    kw = _kw(c)
    kw.pop("src_key")
    zs, zc = c["zs"].to(DEV), c["zc"].to(DEV)
    without = ops.link_rank(zs, zc, *c["args"], _dev(c["target"]), **kw)
    n0, n1 = without[3].cpu().numpy(), c["rank"][n_cand][3].cpu().numpy()
    dense = c["dense"].cpu().numpy()
    hit = 0
    for q in range(n_src):
        ok = _compared(dict(c, skey=np.full(n_src, -1)), q, n_cand) & ~np.isnan(dense[q])
        gone = int((ok & (c["key"] == c["skey"][q])).sum())
        assert n0[q] - n1[q] == gone, q
        hit += gone > 0
    assert hit > 0
    assert torch.equal(without[4].view(torch.int32), c["rank"][n_cand][4].view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_consistent_with_the_filtered_topk(cases, case):
    """No reference involved.  Where the filtered top-k can hold the target at all (its key neither excluded for the
    source nor carried by a second position, which would compete there and not here), the target is among the k
    selected whenever gt + eq < k; it never is when gt >= k."""
    c = cases[case]
    n_src, n_cand = case[:2]
    rank, gt, eq, n, tl = (t.cpu().numpy() for t in c["rank"][n_cand])
    idx = c["topk"][1].cpu().numpy()
    dense = c["dense"].cpu().numpy()
    seen_in = seen_out = 0
    for q in range(n_src):
        p = int(c["target"][q])
        if not 0 <= p < n_cand or np.isnan(tl[q]):
            continue
        if gt[q] >= K:
            assert p not in idx[q], q
            seen_out += 1
        allowed = c["key"][p] != c["skey"][q] and c["key"][p] not in c["ekey"][c["eptr"][q]:c["eptr"][q + 1]]
        if allowed and (c["key"] == c["key"][p]).sum() == 1 and gt[q] + eq[q] < K:
            assert p in idx[q], (q, gt[q], eq[q])
            seen_in += 1
    assert not np.isnan(dense[:, :n_cand]).all()
    if n_src >= 17:
        assert seen_in > 0 and seen_out > 0, (seen_in, seen_out)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_against_the_oracle(cases, case):
    c = cases[case]
    n_src, n_cand = case[:2]
    ref = _ref_logits(c["lins"], c["zs"], c["zc_clean"]).double().numpy()
    rank, gt, eq, n, tl = (t.cpu().numpy() for t in c["rank_clean"])
    rows = _ranked_rows(c, n_cand)
    br = _bracket(c, ref, n_cand, rows)
    scale = max(float(np.abs(ref).max()), 1.0)
    for q in rows:
        lo, hi = br[q]
        print(f"q {q}: {lo} <= gt {gt[q]}, gt + eq {gt[q] + eq[q]} <= {hi}")
        assert lo <= gt[q] and gt[q] + eq[q] <= hi, (q, lo, gt[q], eq[q], hi)
        assert abs(float(tl[q]) - ref[q, c["target"][q]]) <= TOL * scale
        assert n[q] == _compared(c, q, n_cand).sum()
    plain = [q for q in rows if q not in c["tied"]]
    sharp = [q for q in plain if br[q][0] == br[q][1]]
    print(f"bounds coincide on {len(sharp)} of {len(plain)} rows")
    assert 10 * len(sharp) >= 9 * len(plain), (len(sharp), len(plain))


def test_adversarial_pointers_and_targets_stay_inside_the_arrays():
    """validate=False: pointer values beyond nnz, negative ones and a decreasing pair; targets far outside.  The call
    returns, every count is within [0, n_count], and the rows are exact under the kernel's reading of the pointers."""
    from tgnx import ops
    n_src, n_cand, D = 17, 257, 100
    lins = _weights(D, D, seed=22)
    torch.manual_seed(22)
    zs, zc = torch.randn(n_src, D, device=DEV), torch.randn(n_cand, D, device=DEV)
    a = _args(lins)
    keys = np.sort(np.random.default_rng(1).integers(0, n_cand, 40)).astype(np.int64)
    bad = np.linspace(0, 40, n_src + 1).astype(np.int64)
    bad[3], bad[4] = 10 ** 12, -7                                           # beyond nnz; a decreasing pair, negative
    bad[9] = 2 ** 62
    bad[-1] = 41
    target = np.random.default_rng(2).integers(0, n_cand, n_src).astype(np.int64)
    target[5], target[6], target[7] = 2 ** 62, -2 ** 62, 2 ** 31
    with pytest.raises(ValueError):
        ops.link_rank(zs, zc, *a, _dev(target), exclude=(_dev(bad), _dev(keys)))
    rank, gt, eq, n, tl = ops.link_rank(zs, zc, *a, _dev(target), n_count=n_cand - 1, exclude=(_dev(bad), _dev(keys)),
                                        validate=False)
    torch.cuda.synchronize()
    for t in (gt, eq, n):
        assert bool((t >= 0).all()) and bool((t <= n_cand - 1).all())
    assert bool(torch.isnan(tl[5:8]).all()) and bool(torch.isnan(rank[5:8]).all())
    cl = np.clip(bad, 0, 40)
    lo, hi = cl[:-1], np.maximum(cl[1:], cl[:-1])
    ptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(hi - lo, out=ptr[1:])
    segs = np.concatenate([keys[lo[q]:hi[q]] for q in range(n_src)])
    dense = ops.link_topk(zs, zc, *a, 1, sigmoid=False, return_scores=True)[2].cpu().numpy()
    wgt, weq, wn, _ = link_rank_ref(dense, n_cand - 1, target, None, None, ptr, segs)
    assert np.array_equal(gt.cpu().numpy(), wgt) and np.array_equal(eq.cpu().numpy(), weq)
    assert np.array_equal(n.cpu().numpy(), wn)
    out = ops.link_rank(zs, zc, *a, _dev(target), exclude=(_dev(np.linspace(0, 40, n_src + 1).astype(np.int64)),
                                                          _dev(keys[::-1].copy())), validate=False)   # unsorted
    torch.cuda.synchronize()
    assert bool((out[3] >= 0).all()) and bool((out[3] <= n_cand).all())


def test_plain_call_and_module_method():
    """No keys, no exclusions (the kernel without the filter staging), n_count defaulted; LinkPredictor.rank."""
    from tgnx import ops
    from tgnx.nn import LinkPredictor
    n_src, n_cand, D = 33, 515, 32
    torch.manual_seed(5)
    lp = LinkPredictor(D).to(DEV)
    zs, zc = torch.randn(n_src, D, device=DEV), torch.randn(n_cand, D, device=DEV)
    target = torch.randint(0, n_cand, (n_src,), device=DEV)
    zc[7] = zc[target[0]]
    got = lp.rank(zs, zc, target)
    a = [lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias, lp.lin_final.weight, lp.lin_final.bias]
    dense = ops.link_topk(zs, zc, *a, 1, sigmoid=False, return_scores=True)[2].cpu().numpy()
    wgt, weq, wn, wrank = link_rank_ref(dense, n_cand, target.cpu().numpy())
    assert np.array_equal(got[1].cpu().numpy(), wgt) and np.array_equal(got[2].cpu().numpy(), weq)
    assert np.array_equal(got[3].cpu().numpy(), wn) and np.array_equal(got[0].cpu().numpy(), wrank)
    assert (wn == n_cand - 1).all()                               # position keys: only the target itself leaves
    assert weq[0] >= 1 or int(target[0]) == 7                     # the copy of source 0's target row ties with it
    # the dense selection at k = 1: rank 1 without a tie exactly where the target is the top candidate
    top = ops.link_topk(zs, zc, *a, 1, sigmoid=False)[1][:, 0]
    first = (got[1] == 0) & (got[2] == 0)
    assert torch.equal(top[first], target[first])
    empty = ops.link_rank(zs[:0], zc, *a, target[:0])
    assert all(t.numel() == 0 for t in empty)
    none = ops.link_rank(zs, zc[:0], *a, target)                  # no candidates: every row skipped
    assert bool(torch.isnan(none[0]).all()) and bool((none[3] == 0).all())


@pytest.mark.parametrize("case", CASES[1:3], ids=IDS[1:3])
def test_run_to_run_identical_and_graph_capturable(cases, case):
    from tgnx import ops
    c = cases[case]
    n_cand = case[1]
    zs, zc, t = c["zs"].to(DEV), c["zc"].to(DEV), _dev(c["target"])
    kw = dict(_kw(c), validate=False)
    again = ops.link_rank(zs, zc, *c["args"], t, **kw)
    want = c["rank"][n_cand]
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64)  # noqa: E731
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(again, want))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops.link_rank(zs, zc, *c["args"], t, **kw)
    for x in cap:
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(cap[1:], want[1:]))
