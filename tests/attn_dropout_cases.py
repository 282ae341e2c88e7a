"""The attention-dropout cases shared by test_attn_dropout_cpu.py (are the cases non-vacuous?) and
test_gpu_attn_dropout.py (HIP kernels vs the oracle with the same mask injected).  Test infrastructure only: the mask
comes from dropout_ref (numpy) and the attention from oracle.tgn_ref.transformer_attention; nothing of the library is
called.

Shapes are test_gpu_module_ops.py's edge-attention case: 300 destinations, degrees default_rng(H*C).integers(1, 12),
destination 5 without edges and destination 17 with 150 (more edges than a wave has lanes); operands drawn as that
file's _attn_case draws them.  Key modes: 'default' (a destination's key is its row, an edge's key its row) and
'explicit' (40-bit keys from default_rng(7): 300 node keys, then E edge keys — a 32-bit truncation cannot pass)."""
import functools

import numpy as np
import torch

import dropout_ref as dr

N_DST = 300
SHAPES = [(2, 50, True), (1, 256, True), (4, 8, False), (8, 32, True)]      # (H, C, with_e): NR = 2, 4, 1, 4
PS = (0.1, 0.5)
KEY_MODES = ("default", "explicit")
SEED, STREAM = 20240607, 7
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
CASES = [(H, C, with_e, mode, p) for H, C, with_e in SHAPES for mode in KEY_MODES for p in PS]


def degrees(H, C):
    deg = np.random.default_rng(H * C).integers(1, 12, N_DST)
    deg[5], deg[17] = 0, 150
    return deg


@functools.lru_cache(maxsize=None)
def operands(H, C, with_e):
    """(q, k, v, e, indptr, i, dout) on the CPU, fp32; i [E] the destination of every edge row."""
    g = torch.Generator().manual_seed(H * C)
    deg = torch.from_numpy(degrees(H, C))
    E = int(deg.sum())
    indptr = torch.zeros(N_DST + 1, dtype=torch.long)
    indptr[1:] = deg.cumsum(0)
    i = torch.repeat_interleave(torch.arange(N_DST), deg)
    q = torch.randn(N_DST, H * C, generator=g)
    k, v = torch.randn(E, H * C, generator=g), torch.randn(E, H * C, generator=g)
    e = torch.randn(E, H * C, generator=g) if with_e else None
    dout = torch.randn(N_DST, H * C, generator=g)
    return q, k, v, e, indptr, i, dout


def keys(E, mode):
    """(dst_key [300], edge_key [E]) int64 numpy."""
    if mode == "default":
        return np.arange(N_DST, dtype=np.int64), np.arange(E, dtype=np.int64)
    rng = np.random.default_rng(7)
    return rng.integers(0, 2 ** 40, N_DST), rng.integers(0, 2 ** 40, E)


def keep_mask(seed, stream, dkey_per_edge, ekey, H, p):
    """[E, H] float32, 0 or 1 / (1 - p): keep32(drop_base(seed, stream, dkey_i, ekey_p), h)."""
    base = dr.drop_base(seed, stream, np.asarray(dkey_per_edge), np.asarray(ekey))
    return torch.from_numpy(np.stack([dr.keep_scale(base, h, p) for h in range(H)], 1).reshape(-1, H))


def oracle(q, k, v, e, i, n_dst, H, keep, dout):
    """fp32 CPU oracle with the mask injected: (out, alpha, [dq, dk, dv(, de)])."""
    from oracle.tgn_ref import transformer_attention
    C = q.size(1) // H
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v) + ((e,) if e is not None else ())]
    qr, kr, vr = leaves[:3]
    er = leaves[3] if e is not None else torch.zeros_like(kr)
    out, alpha = transformer_attention(qr[i].view(-1, H, C), kr.view(-1, H, C), vr.view(-1, H, C), er.view(-1, H, C),
                                       i, n_dst, keep=keep)
    out.backward(dout)
    return out.detach(), alpha.detach(), [x.grad for x in leaves]


@functools.lru_cache(maxsize=None)
def case(H, C, with_e, mode, p):
    """Operands, keys, the restated mask and the oracle's results with it (and, for the non-vacuity conditions, its
    output without it).  Computed once; nobody writes into it."""
    q, k, v, e, indptr, i, dout = operands(H, C, with_e)
    dkey, ekey = keys(k.size(0), mode)
    keep = keep_mask(SEED, STREAM, dkey[i.numpy()], ekey, H, p)
    out, alpha, grads = oracle(q, k, v, e, i, N_DST, H, keep, dout)
    plain = plain_oracle(H, C, with_e)
    return dict(q=q, k=k, v=v, e=e, indptr=indptr, i=i, dout=dout, dkey=torch.from_numpy(dkey),
                ekey=torch.from_numpy(ekey), keep=keep, out=out, alpha=alpha, grads=grads, plain_out=plain[0])


@functools.lru_cache(maxsize=None)
def plain_oracle(H, C, with_e):
    q, k, v, e, indptr, i, dout = operands(H, C, with_e)
    return oracle(q, k, v, e, i, N_DST, H, None, dout)


def mask_stats(c):
    """From the restated mask alone: the dropped share, how far the mask moves the oracle's output (in close()'s
    measure, max |a - b| over max(|b|_max, 1)), and whether some (destination, head) loses every edge / some with
    >= 2 edges keeps all."""
    keep, i = c["keep"], c["i"]
    H = keep.size(1)
    kept = (keep != 0).long()
    n_kept = torch.zeros(N_DST, H, dtype=torch.long).index_add(0, i, kept)
    deg = torch.bincount(i, minlength=N_DST).view(-1, 1).expand(-1, H)
    scale = max(float(c["plain_out"].abs().max()), 1.0)
    return dict(dropped=float((keep == 0).double().mean()),
                effect=float((c["out"] - c["plain_out"]).abs().max()) / scale,
                all_dropped=bool(((deg >= 1) & (n_kept == 0)).any()),
                all_kept=bool(((deg >= 2) & (n_kept == deg)).any()))


def assert_not_vacuous(c, p):
    s = mask_stats(c)
    assert p / 2 <= s["dropped"] <= 2 * p, s
    assert s["effect"] > 100 * FWD_TOL, s
    if p == 0.5:        # not at 0.1: (1, 256) with explicit keys has no fully dropped pair there
        assert s["all_dropped"] and s["all_kept"], s
    return s
