"""GPU checks of the fused all-pairs LinkPredictor + top-k operator (csrc/tgnx_topk.hip; torch.ops.tgnx.predictor_topk,
tgnx.ops.link_topk, tgnx.nn.LinkPredictor.topk).

The reference is the logits of oracle.tgn_ref.RefLinkPredictor composed on the CPU over all pairs:
lin_final(relu(lin_src(zs)[:, None] + lin_dst(zc)[None])).  Per case:
  * the returned logits match it at 2e-5 in the project's `_close` metric (max |a - b| over max(|b|, 1),
    test_gpu_module_ops.py: the tolerance the predictor op is held to; it covers reassociation only);
  * (idx, val) equal EXACTLY the stable top-k of the returned logits row (np.lexsort((pos, -logit))), padding
    idx -1 / -inf: the selection is bit-for-bit consistent with the logits the same pass wrote;
  * against the reference without assuming equal rounding: with tol = 2e-5 and scale = max(|ref|, 1), every
    selected candidate's reference logit is >= the reference's k-th largest - 2 tol scale (a candidate whose
    computed logit beat the true k-th's can be below it by at most both errors), and the returned values match the
    reference logits at the returned positions within tol scale;
  * sigmoid=True returns the sigmoid of the same selection.
Shapes: one pair; fewer candidates than k (padding); more than one source tile and a partial one, a partial chunk;
200 x 1000 (the 512-candidate chunks are not reached below 256 workgroups: 13 tiles x 20 chunks does, at 10,000
candidates — `test_wide_chunks`); k = 128 = TGNX_TOPK_MAX over 12 chunks; d_in != D; D no multiple of 4; D = 3 (a
row of one 16-byte vector: shorter than the pair loop's load group)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 2e-5

#        n_src, n_cand, d_in, D, k
CASES = [(1, 1, 100, 100, 1), (3, 5, 100, 100, 10), (70, 257, 100, 100, 10), (200, 1000, 100, 100, 64),
         (5, 3000, 32, 32, 128), (4, 300, 48, 100, 7), (17, 600, 30, 30, 5), (3, 300, 5, 3, 2)]


def _weights(d_in, D, seed):
    """RefLinkPredictor's parameters (d_in == D: the oracle module itself; else Linears of its shapes and init)."""
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


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
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


def _check_selection(val, idx, logits, k):
    val, idx, logits = val.cpu().numpy(), idx.cpu().numpy(), logits.cpu().numpy()
    assert val.shape == idx.shape == (logits.shape[0], k)
    for q in range(logits.shape[0]):
        wi, wv = _stable_topk(logits[q], k)
        assert np.array_equal(idx[q], wi), (q, idx[q], wi)
        assert np.array_equal(val[q], wv), (q, val[q], wv)


@pytest.fixture(scope="module")
def cases():
    """Every case's inputs, reference logits and the op's three outputs, computed once and left unchanged."""
    from tgnx import ops
    out = {}
    for c in CASES:
        n_src, n_cand, d_in, D, k = c
        lins = _weights(d_in, D, seed=n_src + n_cand)
        zs, zc = torch.randn(n_src, d_in), torch.randn(n_cand, d_in)
        ref = _ref_logits(lins, zs, zc)
        a = _args(lins)
        got = ops.link_topk(zs.to(DEV), zc.to(DEV), *a, k, sigmoid=False, return_scores=True)
        out[c] = dict(lins=lins, zs=zs, zc=zc, ref=ref, args=a, got=got)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_logits_match_the_oracle(cases, case):
    c = cases[case]
    assert c["got"][2].shape == c["ref"].shape
    _close(c["got"][2], c["ref"], TOL)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_selection_is_the_stable_topk_of_the_returned_logits(cases, case):
    val, idx, logits = cases[case]["got"]
    _check_selection(val, idx, logits, case[4])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_selection_against_the_oracle(cases, case):
    c = cases[case]
    n_src, n_cand, _, _, k = case
    ref = c["ref"].double().numpy()
    val, idx = c["got"][0].cpu().double().numpy(), c["got"][1].cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    kk = min(k, n_cand)
    assert (idx[:, :kk] >= 0).all() and (idx[:, :kk] < n_cand).all() and (idx[:, kk:] == -1).all()
    for q in range(n_src):
        assert len(set(idx[q, :kk].tolist())) == kk                     # k distinct candidates
        kth = np.sort(ref[q])[::-1][kk - 1]
        at = ref[q, idx[q, :kk]]
        assert (at >= kth - 2 * TOL * scale).all(), (q, float((kth - at).max()), 2 * TOL * scale)
        assert np.abs(val[q, :kk] - at).max() <= TOL * scale


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_sigmoid_output_is_the_same_selection(cases, case):
    from tgnx import ops
    c = cases[case]
    val, idx, _ = c["got"]
    sv, si = ops.link_topk(c["zs"].to(DEV), c["zc"].to(DEV), *c["args"], case[4])       # sigmoid=True, no scores
    assert torch.equal(si, idx)
    pad = idx < 0
    assert torch.equal(sv[pad], torch.zeros_like(sv[pad]))
    # 1 / (1 + exp(-x)) in fp32 on both sides: a few ulp of a value in (0, 1]
    assert float((sv[~pad] - torch.sigmoid(val[~pad])).abs().max()) <= 1e-6
    # the order is the logits' even where the sigmoid saturates: not re-sorted by the fp32 sigmoid
    assert bool((sv[:, :-1] >= sv[:, 1:]).all())


def test_wide_chunks_and_a_partial_last_chunk():
    """13 source tiles x 20 chunks of 512 (the wide-chunk path: >= 256 workgroups), last chunk 272 wide."""
    from tgnx import ops
    n_src, n_cand, D, k = 200, 10000, 32, 10
    lins = _weights(D, D, seed=5)
    zs, zc = torch.randn(n_src, D), torch.randn(n_cand, D)
    val, idx, logits = ops.link_topk(zs.to(DEV), zc.to(DEV), *_args(lins), k, sigmoid=False, return_scores=True)
    _close(logits, _ref_logits(lins, zs, zc), TOL)
    _check_selection(val, idx, logits, k)


@pytest.mark.parametrize("kind", ["identical", "scattered"])
def test_ties_go_to_the_lower_position(kind):
    from tgnx import ops
    torch.manual_seed(11)
    D, k = 100, 10
    lins = _weights(D, D, seed=3)
    if kind == "identical":
        zc = torch.randn(1, D).repeat(100, 1)                 # every logit of a row equal: positions 0 .. k - 1
    else:
        # 20 distinct rows copied to scattered positions of three chunks (~35 copies each): every source's k best
        # are copies of its best row, within and across chunks
        zc = torch.randn(20, D)[torch.randint(0, 20, (700,))]
    zs = torch.randn(37, D)
    val, idx, logits = ops.link_topk(zs.to(DEV), zc.to(DEV), *_args(lins), k, sigmoid=False, return_scores=True)
    lg = logits.cpu().numpy()
    if kind == "identical":
        assert (lg == lg[:, :1]).all()
        assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (37, 1)))
    else:
        assert all(np.unique(lg[q]).size <= 20 for q in range(37))
        assert bool((val[:, :1] == val).all())              # the selection sits inside one tie group
        assert int(idx.max()) >= 256                          # and reaches past the first chunk
    _check_selection(val, idx, logits, k)


def test_repeat_call_and_graph_replay_give_the_same_result():
    from tgnx import ops
    torch.manual_seed(2)
    D, k = 100, 10
    lins = _weights(D, D, seed=9)
    zs, zc = torch.randn(70, D, device=DEV), torch.randn(257, D, device=DEV)
    a = _args(lins)
    first = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True)
    again = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops.link_topk(zs, zc, *a, k, sigmoid=False, return_scores=True)
    for t in cap:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(first, cap):
        assert torch.equal(x, y)


def test_link_predictor_module_topk_is_the_op():
    from tgnx import ops
    from tgnx.nn import LinkPredictor
    torch.manual_seed(4)
    lp = LinkPredictor(32).to(DEV)
    zs, zc = torch.randn(9, 32, device=DEV), torch.randn(400, 32, device=DEV)
    val, idx, logits = lp.topk(zs, zc, 6, return_scores=True)
    want = ops.link_topk(zs, zc, lp.lin_src.weight, lp.lin_src.bias, lp.lin_dst.weight, lp.lin_dst.bias,
                         lp.lin_final.weight, lp.lin_final.bias, 6, sigmoid=True, return_scores=True)
    assert torch.equal(val, want[0]) and torch.equal(idx, want[1]) and torch.equal(logits, want[2])
    assert not val.requires_grad and not logits.requires_grad
    v2, i2 = lp.topk(zs, zc, 6)
    assert torch.equal(v2, val) and torch.equal(i2, idx)
    # the module's forward on the selected pairs gives the selected outputs (same weights, the per-pair op)
    pair = lp(zs.repeat_interleave(6, 0), zc[idx.reshape(-1)]).view(9, 6)
    assert float((pair.detach() - val).abs().max()) <= 1e-5


def test_no_candidates_is_all_padding():
    from tgnx import ops
    lins = _weights(32, 32, seed=1)
    zs, zc = torch.randn(5, 32, device=DEV), torch.zeros(0, 32, device=DEV)
    val, idx, logits = ops.link_topk(zs, zc, *_args(lins), 3, sigmoid=False, return_scores=True)
    assert logits.shape == (5, 0)
    assert bool((idx == -1).all()) and bool(torch.isinf(val).all()) and bool((val < 0).all())
    val, idx = ops.link_topk(zs, zc, *_args(lins), 3)
    assert bool((idx == -1).all()) and bool((val == 0).all())
