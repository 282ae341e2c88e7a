"""GPU checks of the filtered and the per-source-list top-k operators (csrc/tgnx_topk.hip;
torch.ops.tgnx.predictor_topk_filtered / predictor_topk_lists, tgnx.ops.link_topk's keywords).

Both are held to the existing operator bit for bit: a pair's logit is one fma chain that does not depend on the grid,
so the filtered operator's logits and the lists operator's ragged logits are torch.equal to ops.link_topk's out_all
on the same inputs, and the selections equal tests/topk_filter_ref.py on those logits exactly.  Against the oracle
(RefLinkPredictor composed over all pairs on the CPU) without assuming equal rounding, as test_gpu_link_topk.py's
third check: with tol = 2e-5 and scale = max(|ref|, 1), every selected candidate's reference logit is >= the
reference's k-th largest OF THE ALLOWED SET - 2 tol scale, and the values are within tol scale.

Shapes (n_src, n_cand, d_in, D, k): the smallest; two source tiles, one partial, and a chunk boundary; D no multiple
of 4; k = 128 over 12 chunks; D = 3 (a row shorter than the pair loop's load group).  Exclusion lists per source, by q mod 4: none; a few keys that hit the first and last
position of a chunk, the last candidate and nothing at all; every candidate (the row is padding; 3,000 keys: past
the LDS staging, searched in global memory); all but a few (k larger than what remains).  cand_key carries a
duplicated node.  List lengths 0, 1, one chunk (256), one chunk + 1, and 3,000 at k = 128; entries -1, entries >=
n_cand, a duplicated entry."""
import numpy as np
import pytest
import torch

from topk_filter_ref import filtered_topk, lists_topk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 2e-5
LCHUNK = 256

#        n_src, n_cand, d_in, D, k
CASES = [(1, 1, 100, 100, 1), (17, 257, 100, 100, 10), (70, 600, 30, 30, 5), (5, 3000, 32, 32, 128),
         (3, 300, 5, 3, 2)]
IDS = ["x".join(map(str, c)) for c in CASES]


def _weights(d_in, D, seed):
    torch.manual_seed(seed)
    if d_in == D:
        from oracle.tgn_ref import RefLinkPredictor
        lp = RefLinkPredictor(D)
        return lp.lin_src, lp.lin_dst, lp.lin_final
    return torch.nn.Linear(d_in, D), torch.nn.Linear(d_in, D), torch.nn.Linear(D, 1)


def _ref_logits(lins, zs, zc):
    ls, ld, lf = lins
    with torch.no_grad():
        return lf((ls(zs)[:, None] + ld(zc)[None]).relu()).squeeze(-1)


def _args(lins):
    ls, ld, lf = lins
    return [t.detach().to(DEV) for t in (ls.weight, ls.bias, ld.weight, ld.bias, lf.weight, lf.bias)]


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long).to(DEV)


def _exclusions(rng, n_src, n_cand, k, key):
    """Ascending segments by q mod 4 (module docstring); keys >= 10**6 match no candidate."""
    segs = []
    for q in range(n_src):
        kind = q % 4 if n_src > 1 else 1
        if kind == 0:
            seg = np.zeros(0, dtype=np.int64)
        elif kind == 1:
            pos = [p for p in (0, LCHUNK - 1, LCHUNK, 2 * LCHUNK - 1, n_cand - 1) if p < n_cand]
            seg = np.concatenate([key[pos], key[pos[:1]], [10 ** 6 + q, 10 ** 6 + q, -5]])   # duplicates, no match
        elif kind == 2:
            seg = key.copy()
        else:
            seg = key[rng.permutation(n_cand)[:max(n_cand - k // 2 - 1, 0)]]
        segs.append(np.sort(seg.astype(np.int64)))
    ptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum([s.size for s in segs], out=ptr[1:])
    return ptr, np.concatenate(segs)


def _lists(rng, n_src, n_cand, k):
    """(ptr, positions): lengths 0, 1, one chunk, one chunk + 1, 40 in turn (3,000 first at k = 128); every longer
    list carries a -1, an entry >= n_cand and a duplicated neighbour pair."""
    lens = [(3000 if k == 128 else 40, 0, 1, LCHUNK, LCHUNK + 1)[q % 5] for q in range(n_src)]
    if n_src == 1:
        lens = [LCHUNK + 1]
    rows = []
    for n in lens:
        r = rng.integers(0, n_cand, n).astype(np.int64)
        if n >= 40:
            r[3] = -1
            r[n - 2] = n_cand + 7
            r[7] = n_cand
            r[11] = r[10]
            r[n - 1] = r[0]
        rows.append(r)
    ptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate(rows)


@pytest.fixture(scope="module")
def cases():
    """Every case's inputs, reference logits, the unfiltered operator's outputs and the two new operators' outputs,
    computed once and left unchanged."""
    from tgnx import ops
    out = {}
    for c in CASES:
        n_src, n_cand, d_in, D, k = c
        rng = np.random.default_rng(n_src + n_cand)
        lins = _weights(d_in, D, seed=n_src + n_cand)
        zs, zc = torch.randn(n_src, d_in), torch.randn(n_cand, d_in)
        a = _args(lins)
        dense = ops.link_topk(zs.to(DEV), zc.to(DEV), *a, k, sigmoid=False, return_scores=True)
        key = rng.permutation(4 * n_cand)[:n_cand].astype(np.int64) + 50
        if n_cand > 1:
            key[n_cand - 1] = key[1]                              # one node at two positions
        skey = np.where(rng.random(n_src) < 0.7, key[rng.integers(0, n_cand, n_src)], -1).astype(np.int64)
        skey[::8] = -1                                            # with q mod 4 == 0: sources without any exclusion
        eptr, ekey = _exclusions(rng, n_src, n_cand, k, key)
        filt = ops.link_topk(zs.to(DEV), zc.to(DEV), *a, k, sigmoid=False, return_scores=True, cand_key=_dev(key),
                             src_key=_dev(skey), exclude=(_dev(eptr), _dev(ekey)))
        lptr, lidx = _lists(rng, n_src, n_cand, k)
        lists = ops.load().predictor_topk_lists(zs.to(DEV), zc.to(DEV), *a, k, False, True, _dev(lptr), _dev(lidx),
                                                int(np.diff(lptr).max()))
        out[c] = dict(lins=lins, zs=zs, zc=zc, ref=_ref_logits(lins, zs, zc), args=a, dense=dense, key=key, skey=skey,
                      eptr=eptr, ekey=ekey, filt=filt, lptr=lptr, lidx=lidx, lists=lists)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ filtered operator
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filtered_logits_are_the_unfiltered_operators_bits(cases, case):
    c = cases[case]
    assert torch.equal(c["filt"][2], c["dense"][2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filtered_selection_is_the_reference_on_those_logits(cases, case):
    c = cases[case]
    val, idx, logits = (t.cpu().numpy() for t in c["filt"])
    wi, wv = filtered_topk(logits, c["key"], c["skey"], c["eptr"], c["ekey"], case[4])
    assert np.array_equal(idx, wi), np.argwhere(idx != wi)[:5]
    assert np.array_equal(val, wv)
    if case[0] > 2:
        # source 1 names the last candidate's key, which position 1 carries too: both are gone, and the chunk edges
        gone = [p for p in (0, 1, LCHUNK - 1, LCHUNK, 2 * LCHUNK - 1, case[1] - 1) if p < case[1]]
        assert not np.isin(idx[1], gone).any()
        assert (idx[2] == -1).all() and np.isneginf(val[2]).all()          # every candidate named: all padding
    if case[0] > 3:
        assert (idx[3] >= 0).sum() < case[4] and (idx[3] >= 0).any()      # k larger than what remains


def _allowed(c, q):
    ok = c["key"] != c["skey"][q]
    return ok & ~np.isin(c["key"], c["ekey"][c["eptr"][q]:c["eptr"][q + 1]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filtered_selection_against_the_oracle(cases, case):
    c = cases[case]
    n_src, n_cand, _, _, k = case
    ref = c["ref"].double().numpy()
    val, idx = c["filt"][0].cpu().double().numpy(), c["filt"][1].cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    for q in range(n_src):
        ok = _allowed(c, q)
        kk = min(k, int(ok.sum()))
        assert (idx[q, kk:] == -1).all() and (idx[q, :kk] >= 0).all() and (idx[q, :kk] < n_cand).all()
        if kk == 0:
            continue
        assert ok[idx[q, :kk]].all(), (q, "an excluded candidate was selected")
        assert len(set(idx[q, :kk].tolist())) == kk
        kth = np.sort(ref[q][ok])[::-1][kk - 1]
        at = ref[q, idx[q, :kk]]
        assert (at >= kth - 2 * TOL * scale).all(), (q, float((kth - at).max()), 2 * TOL * scale)
        assert np.abs(val[q, :kk] - at).max() <= TOL * scale


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sources_without_exclusions_get_the_unfiltered_result(cases, case):
    """The filtered kernel with nothing to exclude, and with exclusions on other rows only."""
    from tgnx import ops
    c = cases[case]
    n_src, n_cand, _, _, k = case
    zs, zc = c["zs"].to(DEV), c["zc"].to(DEV)
    dv, di, _ = c["dense"]
    empty = (torch.zeros(n_src + 1, dtype=torch.long, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV))
    for kw in (dict(exclude=empty), dict(cand_key=_dev(c["key"])), dict(src_key=_dev(np.full(n_src, -9)))):
        got = ops.link_topk(zs, zc, *c["args"], k, sigmoid=False, **kw)
        assert torch.equal(got[0], dv) and torch.equal(got[1], di), kw.keys()
    got = ops.load().predictor_topk_filtered(zs, zc, *c["args"], k, False, False, None, None, None, None)
    assert torch.equal(got[0], dv) and torch.equal(got[1], di)
    free = [q for q in range(n_src) if c["skey"][q] < 0 and c["eptr"][q] == c["eptr"][q + 1]]
    if n_src > 4:
        assert free
    fv, fi, _ = c["filt"]
    assert torch.equal(fv[free], dv[free]) and torch.equal(fi[free], di[free])


def test_self_exclusion_alone_and_position_keys():
    """cand_key None: a candidate's key is its position, here in src_key and in the lists."""
    from tgnx import ops
    n_src, n_cand, D, k = 17, 257, 100, 10
    lins = _weights(D, D, seed=21)
    torch.manual_seed(21)
    zs, zc = torch.randn(n_src, D, device=DEV), torch.randn(n_cand, D, device=DEV)
    a = _args(lins)
    dv, di, lg = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True)
    best = di[:, 0].cpu().numpy()
    val, idx, lg2 = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True, src_key=_dev(best))
    assert torch.equal(lg2, lg)
    wi, wv = filtered_topk(lg.cpu().numpy(), None, best, None, None, k)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), wv)
    assert torch.equal(idx[:, :k - 1], di[:, 1:])                          # the best one left, the rest moved up
    # the same exclusions as one-key lists; then the first and last position of both chunks for every source
    ptr = np.arange(n_src + 1)
    v2, i2 = ops.link_topk(zs, zc, *a, k, sigmoid=False, exclude=(_dev(ptr), _dev(best)))
    assert torch.equal(v2, val) and torch.equal(i2, idx)
    edge = np.array([0, 255, 256], dtype=np.int64)
    v3, i3 = ops.link_topk(zs, zc, *a, k, sigmoid=False, exclude=(_dev(ptr * 3), _dev(np.tile(edge, n_src))))
    wi, wv = filtered_topk(lg.cpu().numpy(), None, None, ptr * 3, np.tile(edge, n_src), k)
    assert np.array_equal(i3.cpu().numpy(), wi) and np.array_equal(v3.cpu().numpy(), wv)
    assert not np.isin(i3.cpu().numpy(), edge).any()


def test_adversarial_pointers_stay_inside_the_arrays():
    """validate=False: pointer values beyond nnz, negative ones and a decreasing pair; an unsorted segment.  The calls
    succeed, every selected position is in range, and the rows whose segments are well-formed are exact."""
    from tgnx import ops
    n_src, n_cand, D, k = 17, 257, 100, 10
    lins = _weights(D, D, seed=22)
    torch.manual_seed(22)
    zs, zc = torch.randn(n_src, D, device=DEV), torch.randn(n_cand, D, device=DEV)
    a = _args(lins)
    keys = np.sort(np.random.default_rng(1).integers(0, n_cand, 40)).astype(np.int64)
    ptr = np.linspace(0, 40, n_src + 1).astype(np.int64)
    bad = ptr.copy()
    bad[3], bad[4] = 10 ** 12, -7                                           # beyond nnz; a decreasing pair, negative
    bad[9] = 2 ** 62
    bad[-1] = 41
    with pytest.raises(ValueError):
        ops.link_topk(zs, zc, *a, k, sigmoid=False, exclude=(_dev(bad), _dev(keys)))
    val, idx, lg = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True, exclude=(_dev(bad), _dev(keys)),
                                 validate=False)
    torch.cuda.synchronize()
    assert bool((idx >= -1).all()) and bool((idx < n_cand).all())
    # the kernel's reading: values clamped into [0, nnz], a decreasing pair an empty segment
    cl = np.clip(bad, 0, 40)
    lo, hi = cl[:-1], np.maximum(cl[1:], cl[:-1])
    for q in range(n_src):
        wi, wv = filtered_topk(lg[q:q + 1].cpu().numpy(), None, None, [0, hi[q] - lo[q]], keys[lo[q]:hi[q]], k)
        assert np.array_equal(idx[q].cpu().numpy(), wi[0]), q
    shuffled = keys[::-1].copy()
    with pytest.raises(ValueError):
        ops.link_topk(zs, zc, *a, k, sigmoid=False, exclude=(_dev(ptr), _dev(shuffled)))
    val, idx = ops.link_topk(zs, zc, *a, k, sigmoid=False, exclude=(_dev(ptr), _dev(shuffled)), validate=False)
    torch.cuda.synchronize()
    assert bool((idx >= -1).all()) and bool((idx < n_cand).all())
    # the lists operator under the same pointers
    pos = _dev(np.random.default_rng(2).integers(-1, n_cand + 2, 40))
    out = ops.link_topk(zs, zc, *a, k, sigmoid=False, lists=(_dev(bad), pos), validate=False)
    torch.cuda.synchronize()
    assert bool((out[1] >= -1).all()) and bool((out[1] < n_cand).all())
    assert bool((out[2] >= -1).all()) and bool((out[2] < 40).all())


# --------------------------------------------------------------------------------------------------- lists operator
def _entry_rows(lptr):
    return np.repeat(np.arange(len(lptr) - 1), np.diff(lptr))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_list_logits_are_the_dense_operators_bits(cases, case):
    c = cases[case]
    n_cand = case[1]
    val, idx, slot, logits, bad = c["lists"]
    lidx, rows = c["lidx"], _entry_rows(c["lptr"])
    valid = (lidx >= 0) & (lidx < n_cand)
    assert int(bad) == int((lidx >= n_cand).sum())
    lg = logits.cpu()
    assert bool(torch.isnan(lg[torch.from_numpy(~valid)]).all())
    want = c["dense"][2].cpu()[torch.from_numpy(rows[valid]), torch.from_numpy(lidx[valid])]
    assert torch.equal(lg[torch.from_numpy(valid)], want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_list_selection_is_the_reference_on_those_logits(cases, case):
    c = cases[case]
    k = case[4]
    val, idx, slot, logits, _ = (t.cpu().numpy() for t in c["lists"])
    ws, wv = lists_topk(logits, c["lptr"], k)
    assert np.array_equal(slot, ws), np.argwhere(slot != ws)[:5]
    assert np.array_equal(val, wv)
    at = c["lptr"][:-1, None] + np.maximum(slot, 0)
    assert np.array_equal(idx, np.where(slot >= 0, c["lidx"][np.minimum(at, len(c["lidx"]) - 1)], -1))
    for q in range(case[0]):                                               # the duplicated pair: lower slot first
        if c["lptr"][q + 1] - c["lptr"][q] >= 40 and 10 in slot[q]:
            r = int(np.flatnonzero(slot[q] == 10)[0])
            assert r + 1 == k or slot[q, r + 1] == 11


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_list_selection_against_the_oracle(cases, case):
    c = cases[case]
    n_src, n_cand, _, _, k = case
    ref = c["ref"].double().numpy()
    val, idx, slot = (c["lists"][i].cpu().numpy() for i in range(3))
    scale = max(float(np.abs(ref).max()), 1.0)
    for q in range(n_src):
        ent = c["lidx"][c["lptr"][q]:c["lptr"][q + 1]]
        ok = (ent >= 0) & (ent < n_cand)
        kk = min(k, int(ok.sum()))
        assert (slot[q, kk:] == -1).all() and (idx[q, kk:] == -1).all()
        if kk == 0:
            continue
        assert ok[slot[q, :kk]].all() and len(set(slot[q, :kk].tolist())) == kk
        kth = np.sort(ref[q, ent[ok]])[::-1][kk - 1]
        at = ref[q, idx[q, :kk]]
        assert (at >= kth - 2 * TOL * scale).all(), (q, float((kth - at).max()), 2 * TOL * scale)
        assert np.abs(val[q, :kk].astype(np.float64) - at).max() <= TOL * scale


def test_list_entries_past_max_len_are_skipped_and_counted():
    from tgnx import ops
    n_src, n_cand, D, k = 5, 300, 32, 6
    lins = _weights(D, D, seed=23)
    torch.manual_seed(23)
    zs, zc = torch.randn(n_src, D, device=DEV), torch.randn(n_cand, D, device=DEV)
    a = _args(lins)
    lens = np.array([0, 1, 100, 101, 3 * LCHUNK + 5])
    ptr = np.concatenate([[0], np.cumsum(lens)])
    pos = np.random.default_rng(3).integers(0, n_cand, int(lens.sum()))
    full = ops.load().predictor_topk_lists(zs, zc, *a, k, False, True, _dev(ptr), _dev(pos), int(lens.max()))
    assert int(full[4]) == 0
    for max_len in (100, 0):                                               # one chunk; the sweep past the grid
        val, idx, slot, logits, bad = ops.load().predictor_topk_lists(zs, zc, *a, k, False, True, _dev(ptr), _dev(pos),
                                                                      max_len)
        off = np.arange(int(lens.sum())) - ptr[_entry_rows(ptr)]
        cut = torch.from_numpy(off >= max_len)
        assert int(bad) == int(cut.sum())
        lg = logits.cpu()
        assert bool(torch.isnan(lg[cut]).all()) and torch.equal(lg[~cut], full[3].cpu()[~cut])
        ws, wv = lists_topk(lg.numpy(), ptr, k)
        assert np.array_equal(slot.cpu().numpy(), ws) and np.array_equal(val.cpu().numpy(), wv)
        assert int(slot.max()) < max_len
    # link_topk: the bound is the longest list when validated, len(positions) otherwise
    for validate in (True, False):
        got = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True, lists=(_dev(ptr), _dev(pos)),
                            validate=validate)
        assert all(torch.equal(x, y) for x, y in zip(got, full[:4]))


def test_no_sources_and_no_candidates():
    from tgnx import ops
    lins = _weights(32, 32, seed=1)
    a = _args(lins)
    zc = torch.randn(9, 32, device=DEV)
    none = torch.zeros(0, 32, device=DEV)
    zero = torch.zeros(1, dtype=torch.long, device=DEV)
    out = ops.link_topk(none, zc, *a, 3, lists=(zero, torch.zeros(0, dtype=torch.long, device=DEV)))
    assert all(t.shape == (0, 3) for t in out)
    out = ops.link_topk(none, zc, *a, 3, exclude=(zero, torch.zeros(0, dtype=torch.long, device=DEV)))
    assert all(t.shape == (0, 3) for t in out)
    zs = torch.randn(4, 32, device=DEV)
    ptr, pos = _dev([0, 2, 2, 3, 5]), _dev([0, 3, -1, 1, 0])
    val, idx, slot, logits, bad = ops.load().predictor_topk_lists(zs, none, *a, 3, True, True, ptr, pos, 2)
    assert int(bad) == 4 and bool(torch.isnan(logits).all())              # no candidates: every entry >= n_cand
    assert bool((idx == -1).all()) and bool((slot == -1).all()) and bool((val == 0).all())


# ------------------------------------------------------------------------------------------------- both operators
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sigmoid_and_repeat_calls(cases, case):
    from tgnx import ops
    c = cases[case]
    k = case[4]
    zs, zc = c["zs"].to(DEV), c["zc"].to(DEV)
    kw = dict(cand_key=_dev(c["key"]), src_key=_dev(c["skey"]), exclude=(_dev(c["eptr"]), _dev(c["ekey"])))
    again = ops.link_topk(zs, zc, *c["args"], k, sigmoid=False, return_scores=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(again, c["filt"]))
    lagain = ops.link_topk(zs, zc, *c["args"], k, sigmoid=False, return_scores=True,
                           lists=(_dev(c["lptr"]), _dev(c["lidx"])))
    assert torch.equal(lagain[0], c["lists"][0]) and torch.equal(lagain[1], c["lists"][1])
    assert torch.equal(lagain[2], c["lists"][2])
    assert torch.equal(lagain[3].view(torch.int32), c["lists"][3].view(torch.int32))            # NaNs included
    for (sv, si), (val, idx) in ((ops.link_topk(zs, zc, *c["args"], k, **kw), c["filt"][:2]),
                                 (ops.link_topk(zs, zc, *c["args"], k, lists=(_dev(c["lptr"]), _dev(c["lidx"])))[:2],
                                  c["lists"][:2])):
        assert torch.equal(si, idx)
        pad = idx < 0
        assert torch.equal(sv[pad], torch.zeros_like(sv[pad]))
        if bool((~pad).any()):
            assert float((sv[~pad] - torch.sigmoid(val[~pad])).abs().max()) <= 1e-6
        assert bool((sv[:, :-1] >= sv[:, 1:]).all())


def test_graph_replay_gives_the_same_result(cases):
    """Both operators captured into one HIP graph (no host synchronisation, no allocation outside torch's pool)."""
    from tgnx import ops
    case = CASES[1]
    c = cases[case]
    k = case[4]
    zs, zc = c["zs"].to(DEV), c["zc"].to(DEV)
    kw = dict(cand_key=_dev(c["key"]), src_key=_dev(c["skey"]), exclude=(_dev(c["eptr"]), _dev(c["ekey"])),
              validate=False)
    lists = (_dev(c["lptr"]), _dev(c["lidx"]))
    longest = int(np.diff(c["lptr"]).max())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f = ops.link_topk(zs, zc, *c["args"], k, sigmoid=False, return_scores=True, **kw)
        ls = ops.link_topk(zs, zc, *c["args"], k, sigmoid=False, return_scores=True, lists=lists, validate=False,
                           max_len=longest)
    for t in f + ls:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(f, c["filt"]))
    assert all(torch.equal(x, y) for x, y in zip(ls[:3], c["lists"][:3]))
    assert torch.equal(ls[3].view(torch.int32), c["lists"][3].view(torch.int32))


def test_link_predictor_module_forwards_the_keywords():
    from tgnx import ops
    from tgnx.nn import LinkPredictor
    torch.manual_seed(4)
    lp = LinkPredictor(32).to(DEV)
    zs, zc = torch.randn(9, 32, device=DEV), torch.randn(400, 32, device=DEV)
    w = (lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias, lp.lin_final.weight,
         lp.lin_final.bias)
    sk = torch.arange(9, device=DEV)
    ex = (_dev(np.arange(10) * 2), _dev(np.tile([5, 7], 9)))
    got = lp.topk_filtered(zs, zc, 6, return_scores=True, src_key=sk, exclude=ex)
    want = ops.link_topk(zs, zc, *w, 6, sigmoid=True, return_scores=True, src_key=sk, exclude=ex)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not np.isin(got[1].cpu().numpy(), [5, 7]).any()
    ls = (_dev(np.arange(10) * 3), _dev(np.tile([5, 399, 7], 9)))
    got = lp.topk_filtered(zs, zc, 2, lists=ls)
    want = ops.link_topk(zs, zc, *w, 2, sigmoid=True, lists=ls)
    assert len(got) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))
    plain = lp.topk_filtered(zs, zc, 6)
    assert all(torch.equal(x, y) for x, y in zip(plain, lp.topk(zs, zc, 6)))
