"""GPU tests of the leave-one-out link logit operator alone (tgnx_link_predictor_loo; ops.link_loo;
tgnx.nn.LinkPredictor.loo): random embeddings z [7, D], leave-one-out rows loo_z [7, 3, D] and counts in [0, 3] for 7
unique nodes, 13 pairs with repeated rows and pairs naming one node on both sides, D in {2, 32, 100}.

  float64    base, src_logit and dst_logit against the float64 restatement at 2e-5 absolute (the engine's OUT_TOL;
             inputs and weights are scaled so that the logits are of magnitude ~1);
  past count entries with j >= count of the varied node equal base bit for bit;
  order      the pairs shuffled give the unshuffled result, permuted, bit for bit; two calls are bit-identical;
  bad index  a row index outside [0, n) gives NaN for its pair, status 1, and leaves every other pair's bits alone;
  module     LinkPredictor.loo is the operator with the module's parameters."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NN, K, P = 7, 3, 13
TOL = 2e-5


def _case(D, seed=0):
    g = torch.Generator().manual_seed(seed + D)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    z, loo = r(NN, D), r(NN, K, D)
    count = torch.tensor([0, 3, 1, 2, 3, 0, 2], dtype=torch.int32)
    sc = 1.0 / np.sqrt(D)
    w = dict(w_src=r(D, D) * sc, b_src=r(D) * 0.1, w_dst=r(D, D) * sc, b_dst=r(D) * 0.1, w_out=r(1, D) * sc, b_out=r(1))
    src = torch.tensor([0, 1, 1, 2, 3, 4, 4, 5, 6, 6, 3, 1, 0])
    dst = torch.tensor([1, 1, 4, 2, 0, 4, 6, 5, 3, 6, 3, 4, 5])          # repeated rows, and src == dst six times
    return z, loo, count, src, dst, w


def _ref64(z, loo, count, src, dst, w):
    d = {k: v.double() for k, v in w.items()}
    z, loo = z.double(), loo.double()

    def logit(a, b):
        h = (a @ d["w_src"].T + d["b_src"] + b @ d["w_dst"].T + d["b_dst"]).relu()
        return h @ d["w_out"].view(-1) + d["b_out"]

    base = logit(z[src], z[dst])
    sl, dl = base.view(-1, 1).repeat(1, K), base.view(-1, 1).repeat(1, K)
    for p in range(src.numel()):
        s, t = int(src[p]), int(dst[p])
        for j in range(int(count[s])):
            sl[p, j] = logit(loo[s, j][None], z[t][None])
        for j in range(int(count[t])):
            dl[p, j] = logit(z[s][None], loo[t, j][None])
    return base, sl, dl


def _run(z, loo, count, src, dst, w):
    from tgnx import ops
    out = ops.link_loo(z.to(DEV), loo.to(DEV), count.to(DEV), src, dst, w["w_src"].to(DEV), w["b_src"].to(DEV),
                       w["w_dst"].to(DEV), w["b_dst"].to(DEV), w["w_out"].to(DEV), w["b_out"].to(DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D", [2, 32, 100])
def test_against_float64_and_past_count_and_order(D):
    z, loo, count, src, dst, w = _case(D)
    base, sl, dl, status = _run(z, loo, count, src, dst, w)
    assert base.shape == (P,) and sl.shape == dl.shape == (P, K) and int(status) == 0
    want = _ref64(z, loo, count, src, dst, w)
    for name, got, ref in zip(("base", "src", "dst"), (base, sl, dl), want):
        err = float((got.double().cpu() - ref).abs().max())
        print(f"D={D} {name}: max err {err:.3e} scale {float(ref.abs().max()):.3e}")
        assert err <= TOL, (name, err)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    cs, cd = count[src].to(DEV), count[dst].to(DEV)
    j = torch.arange(K, device=DEV)
    for tab, c in ((sl, cs), (dl, cd)):
        past = j[None] >= c[:, None]
        assert bool(past.any()) and torch.equal(bits(tab)[past], bits(base)[:, None].expand(-1, K)[past])
    # src == dst: each side is varied alone (the two tables differ where the node has rows)
    same = (src == dst).to(DEV) & (cs > 0)
    assert bool(same.any()) and not torch.equal(sl[same], dl[same])
    # the pairs shuffled: the same bits, permuted; and the same call again
    perm = torch.from_numpy(np.random.default_rng(D).permutation(P))
    b2, s2, d2, _ = _run(z, loo, count, src[perm], dst[perm], w)
    pd = perm.to(DEV)
    assert torch.equal(bits(b2), bits(base[pd])) and torch.equal(bits(s2), bits(sl[pd])) and torch.equal(bits(d2), bits(dl[pd]))
    b3, s3, d3, _ = _run(z, loo, count, src, dst, w)
    assert torch.equal(bits(b3), bits(base)) and torch.equal(bits(s3), bits(sl)) and torch.equal(bits(d3), bits(dl))


def test_row_index_out_of_range_sets_the_status_and_writes_nan():
    z, loo, count, src, dst, w = _case(32)
    base, sl, dl, _ = _run(z, loo, count, src, dst, w)
    src2, dst2 = src.clone(), dst.clone()
    src2[2], dst2[5], src2[9] = -1, NN, NN + 1000
    b2, s2, d2, status = _run(z, loo, count, src2, dst2, w)
    assert int(status) == 1
    bad = torch.zeros(P, dtype=torch.bool, device=DEV)
    bad[[2, 5, 9]] = True
    assert bool(torch.isnan(b2[bad]).all()) and bool(torch.isnan(s2[bad]).all()) and bool(torch.isnan(d2[bad]).all())
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(b2[~bad]), bits(base[~bad])) and torch.equal(bits(s2[~bad]), bits(sl[~bad]))
    assert torch.equal(bits(d2[~bad]), bits(dl[~bad]))


def test_empty_and_argument_errors():
    from tgnx import ops
    z, loo, count, src, dst, w = _case(32)
    e = torch.empty(0, dtype=torch.long)
    base, sl, dl, status = _run(z, loo, count, e, e, w)
    assert base.shape == (0,) and sl.shape == (0, K) and int(status) == 0
    a = [w[k].to(DEV) for k in ("w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out")]
    with pytest.raises(ValueError, match="link_loo"):
        ops.link_loo(z.to(DEV), loo.to(DEV), count.to(DEV), src, dst[:5], *a)
    with pytest.raises(ValueError, match="link_loo"):
        ops.link_loo(z.to(DEV), loo[:, :, :31].contiguous().to(DEV), count.to(DEV), src, dst, *a)
    with pytest.raises(RuntimeError):          # the op's own check: a weight of another width
        ops.link_loo(z.to(DEV), loo.to(DEV), count.to(DEV), src, dst, a[0][:, :31].contiguous(), *a[1:])


def test_module_wrapper():
    from tgnx.nn import LinkPredictor
    z, loo, count, src, dst, w = _case(32)
    lp = LinkPredictor(32).to(DEV)
    with torch.no_grad():
        lp.lin_src.weight.copy_(w["w_src"]), lp.lin_src.bias.copy_(w["b_src"])
        lp.lin_dst.weight.copy_(w["w_dst"]), lp.lin_dst.bias.copy_(w["b_dst"])
        lp.lin_final.weight.copy_(w["w_out"]), lp.lin_final.bias.copy_(w["b_out"])
    got = lp.loo(z.to(DEV), loo.to(DEV), count.to(DEV), src, dst)
    want = _run(z, loo, count, src, dst, w)
    for g, x in zip(got, want):
        assert torch.equal(g, x)
