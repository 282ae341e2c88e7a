"""Float64 restatements of the per-operator layer (torch.ops.tgnx.* / tgnx/ops.py autograd functions) and the
shape lists of the width sweep, shared by test_module_ref_cpu.py (fp32 CPU vs float64: are the inputs well
conditioned?) and test_gpu_module_widths.py (HIP kernels vs float64).

Every `*_ref` function is dtype-generic: it computes in the dtype of the tensors it is handed, so the same code
is the float64 reference and, on float32 inputs, the fp32 CPU computation the conditioning test measures.  The
oracle is used where it is dtype-generic (oracle.tgn_ref.transformer_attention, last_aggregate, mean_aggregate);
the cells, the predictor, the time encoder and the time embedding are the plain formulas (the cells are pinned to
torch.nn.GRUCell / RNNCell(...).double() in test_module_ref_cpu.py).

Error measure (the project's own, unchanged): max |a - b| over max(|b|_max, 1)."""
import functools
import math

import numpy as np
import torch

FWD_TOL, GRAD_TOL = 2e-5, 1e-4


# ------------------------------------------------------------------ the error measure
def rel_err(a, b):
    """max |a - b| / max(|b|_max, 1) with b the reference; 0 for empty tensors."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    return err, scale


def close(a, b, tol, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = rel_err(a, b)
    print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e} tol {tol:g}")
    assert err <= tol * scale, (what, err, scale)


def run_ref(fn, inputs, dout, dtype):
    """fn(*inputs) in `dtype` with every floating input a leaf: (out, [grad per input, None for non-float])."""
    leaves = [x.detach().to(dtype).requires_grad_(True) if x is not None and x.is_floating_point() else x
              for x in inputs]
    out = fn(*leaves)
    out.backward(dout.to(dtype))
    return out.detach(), [x.grad if x is not None and x.is_floating_point() else None for x in leaves]


# ------------------------------------------------------------------ edge attention
ATTN_HC = [(1, 1), (8, 1), (7, 9), (1, 64), (2, 32), (5, 13), (1, 65), (3, 43), (8, 16), (1, 128), (3, 64), (1, 129),
           (5, 51), (8, 32), (2, 128), (1, 256)]
ATTN_Q_SCALES = (1.0, 8.0)


def attn_degrees(pattern):
    """'main': [0, 1, 2, 63, 64, 65, 150] + 30 degrees from 1..11 (37 destinations: a last block with one live
    wave); 'one': a single destination; 'empty': 37 destinations without any edge (E = 0)."""
    if pattern == "main":
        return [0, 1, 2, 63, 64, 65, 150] + np.random.default_rng(37).integers(1, 12, 30).tolist()
    if pattern == "one":
        return [5]
    assert pattern == "empty"
    return [0] * 37


ATTN_PATTERNS = ("main", "one", "empty")


def attn_ref(H):
    from oracle.tgn_ref import transformer_attention

    def fn(q, k, v, e, indptr):
        n_dst, C = q.size(0), q.size(1) // H
        i = torch.repeat_interleave(torch.arange(n_dst), indptr[1:] - indptr[:-1])
        ee = e if e is not None else torch.zeros_like(k)
        out, alpha = transformer_attention(q[i].view(-1, H, C), k.view(-1, H, C), v.view(-1, H, C), ee.view(-1, H, C),
                                           i, n_dst)
        fn.alpha = alpha.detach()
        return out
    return fn


@functools.lru_cache(maxsize=None)
def attn_case(H, C, with_e, pattern, q_scale):
    """fp32 inputs (q, k, v, e, indptr), dout, and the float64 (out, alpha, [dq, dk, dv, de])."""
    g = torch.Generator().manual_seed(1000 * H + C + (7 if with_e else 0))
    deg = torch.tensor(attn_degrees(pattern), dtype=torch.long)
    n_dst, E, HC = deg.numel(), int(deg.sum()), H * C
    indptr = torch.zeros(n_dst + 1, dtype=torch.long)
    indptr[1:] = deg.cumsum(0)
    q = torch.randn(n_dst, HC, generator=g) * q_scale
    k, v = torch.randn(E, HC, generator=g), torch.randn(E, HC, generator=g)
    e = torch.randn(E, HC, generator=g) if with_e else None
    dout = torch.randn(n_dst, HC, generator=g)
    inputs = (q, k, v, e, indptr)
    fn = attn_ref(H)
    out, grads = run_ref(fn, inputs, dout, torch.float64)
    return dict(inputs=inputs, dout=dout, deg=deg, out=out, alpha=fn.alpha, grads=grads[:4])


# ------------------------------------------------------------------ column sums
COL_SUM_MN = [(M, N) for M in (255, 256, 257, 512, 513) for N in (1, 63, 64, 65, 129)]


def col_sum_case(M, N):
    return torch.randn(M, N, generator=torch.Generator().manual_seed(M * 131 + N))


# ------------------------------------------------------------------ memory cell
CELL_SHAPES = [(1, 1, 1), (5, 3, 2), (256, 64, 64), (257, 65, 63), (255, 129, 65), (7, 300, 128), (3, 17, 172)]
CELL_NO_BIAS = ("gru", 5, 3, 2)


def cell_ref(cell):
    def fn(x, h, w_ih, w_hh, b_ih, b_hh):
        gi = x @ w_ih.t() + (b_ih if b_ih is not None else 0)
        gh = h @ w_hh.t() + (b_hh if b_hh is not None else 0)
        if cell == "rnn":
            return torch.tanh(gi + gh)
        D = h.size(1)
        r = torch.sigmoid(gi[:, :D] + gh[:, :D])
        z = torch.sigmoid(gi[:, D:2 * D] + gh[:, D:2 * D])
        n = torch.tanh(gi[:, 2 * D:] + r * gh[:, 2 * D:])
        return (h - n) * z + n
    return fn


@functools.lru_cache(maxsize=None)
def cell_case(cell, M, d_in, D, bias=True):
    """Parameters drawn as torch.nn.GRUCell / RNNCell draws them: U(-1/sqrt(D), 1/sqrt(D))."""
    g = torch.Generator().manual_seed(M * 7 + d_in * 3 + D + (0 if cell == "gru" else 1))
    G, s = (3 if cell == "gru" else 1) * D, 1.0 / math.sqrt(D)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * s  # noqa: E731
    x, h = torch.randn(M, d_in, generator=g), torch.randn(M, D, generator=g)
    w_ih, w_hh = u(G, d_in), u(G, D)
    b_ih, b_hh = (u(G), u(G)) if bias else (None, None)
    dout = torch.randn(M, D, generator=g)
    inputs = (x, h, w_ih, w_hh, b_ih, b_hh)
    out, grads = run_ref(cell_ref(cell), inputs, dout, torch.float64)
    return dict(inputs=inputs, dout=dout, out=out, grads=grads)


# ------------------------------------------------------------------ link predictor
PRED_D = (1, 2, 63, 64, 65, 129, 172)
PRED_SRC_K = ((1, 1), (3, 5), (257, 1))
PRED_CASES = [(D, D, n_src, k) for D in PRED_D for n_src, k in PRED_SRC_K] + [(20, 65, 3, 5)]   # (d_in, D, n_src, k)
PRED_RELU_MARGIN = 2e-6     # no pre-activation this close to the ReLU's kink (see pred_case)


def pred_ref(sigmoid):
    def fn(z_src, z_dst, w_src, b_src, w_dst, b_dst, w_out, b_out):
        n_src, M = z_src.size(0), z_dst.size(0)
        hs = z_src @ w_src.t() + b_src
        hd = z_dst @ w_dst.t() + b_dst
        pre = hs[torch.arange(M) % n_src] + hd               # row i pairs with source i mod n_src
        fn.pre = pre.detach()
        out = pre.relu() @ w_out.view(-1, 1) + b_out
        return out.sigmoid() if sigmoid else out
    return fn


@functools.lru_cache(maxsize=None)
def pred_case(d_in, D, n_src, k, sigmoid):
    """Parameters as torch.nn.Linear draws them.  The ReLU's gradient is discontinuous at 0: a pre-activation within
    rounding of 0 would make the gradient depend on the summation order, so the seed is advanced until none is
    within PRED_RELU_MARGIN (the conditioning test asserts the margin); `margin` is the smallest |pre-activation|."""
    M = n_src * k
    for attempt in range(16):
        g = torch.Generator().manual_seed(d_in * 1009 + D * 31 + n_src * 5 + k + 100003 * attempt)
        s, so = 1.0 / math.sqrt(d_in), 1.0 / math.sqrt(D)
        u = lambda sc, *shape: (torch.rand(*shape, generator=g) * 2 - 1) * sc  # noqa: E731
        inputs = (torch.randn(n_src, d_in, generator=g), torch.randn(M, d_in, generator=g), u(s, D, d_in), u(s, D),
                  u(s, D, d_in), u(s, D), u(so, 1, D), u(so, 1))
        dout = torch.randn(M, 1, generator=g)
        fn = pred_ref(sigmoid)
        out, grads = run_ref(fn, inputs, dout, torch.float64)
        margin = float(fn.pre.abs().min())
        if margin > PRED_RELU_MARGIN:
            break
    return dict(inputs=inputs, dout=dout, out=out, grads=grads, margin=margin)


# ------------------------------------------------------------------ linear, time encoder, time embedding
ROW_D = (1, 63, 64, 65, 172)
ROW_N = (1, 255, 257)
LINEAR_CASES = [(n, D, D, True) for D in ROW_D for n in ROW_N] + [(257, 65, 129, True), (257, 65, 129, False)]


def linear_ref(x, w, b):
    return x @ w.t() + (b if b is not None else 0)


@functools.lru_cache(maxsize=None)
def linear_case(M, d_in, d_out, bias):
    g = torch.Generator().manual_seed(M * 3 + d_in * 7 + d_out)
    s = 1.0 / math.sqrt(d_in)
    x = torch.randn(M, d_in, generator=g)
    w = (torch.rand(d_out, d_in, generator=g) * 2 - 1) * s
    b = (torch.rand(d_out, generator=g) * 2 - 1) * s if bias else None
    dout = torch.randn(M, d_out, generator=g)
    out, grads = run_ref(linear_ref, (x, w, b), dout, torch.float64)
    return dict(inputs=(x, w, b), dout=dout, out=out, grads=grads)


def time_arg32(t, w, b):
    """The kernels' argument fmaf(w, t, b): w t is exact in float64 (24 + 24 bits), + b and the rounding to float32
    are the two roundings of RefTimeEncoder (with b = 0: the once-rounded float32 product exactly)."""
    return (t.double().view(-1, 1) * w.double().view(1, -1) + b.double().view(1, -1)).float()


def time_encode_ref(t, w, b, dout, dtype):
    """(out, dw, db) in `dtype`, every one a function of the float32 argument: out = cos(arg),
    dw = Σ_n -sin(arg) t dout, db = Σ_n -sin(arg) dout."""
    arg = time_arg32(t, w, b).to(dtype)
    g = -torch.sin(arg) * dout.to(dtype)
    return torch.cos(arg), (g * t.to(dtype).view(-1, 1)).sum(0).view(w.shape), g.sum(0)


@functools.lru_cache(maxsize=None)
def time_encode_case(n, D):
    """Integer timestamps up to 2.6e6 (tgbl-wiki's range), w and b as Linear(1, D) draws them (U(-1, 1))."""
    g = torch.Generator().manual_seed(n * 11 + D)
    t = torch.randint(0, 2_600_000, (n,), generator=g).float()
    w, b = torch.rand(D, 1, generator=g) * 2 - 1, torch.rand(D, generator=g) * 2 - 1
    dout = torch.randn(n, D, generator=g)
    out, dw, db = time_encode_ref(t, w, b, dout, torch.float64)
    return dict(inputs=(t, w, b), dout=dout, out=out, grads=[dw, db])


BIG_N, BIG_D = 257, 65


@functools.lru_cache(maxsize=None)
def time_encode_big_case():
    """n = 257, D = 65, b = 0; t integer-valued up to 2^30; column c's w is ± 2^(-30 c / 64) (1 - u / 4) with u in
    [0, 1) and alternating sign, so that |w t| runs from 0 up to 2^30 with both signs and never reaches 2^31.  The
    argument is computed by numpy's float32 multiply: one rounding, the kernel's fmaf(w, t, 0) bit for bit."""
    rng = np.random.default_rng(2030)
    t = np.concatenate([[0.0, 1.0, 2.0 ** 30, 2.0 ** 30 - 64.0],
                        np.floor(2.0 ** rng.uniform(0, 30, BIG_N - 4))]).astype(np.float32)
    assert t.max() <= 2.0 ** 30 and np.all(t == np.floor(t))
    mag = 2.0 ** (-30.0 * np.arange(BIG_D) / (BIG_D - 1)) * (1.0 - rng.uniform(0, 0.25, BIG_D))
    mag[0] = 1.0                                             # |w t| reaches 2^30 exactly
    w = (mag * np.where(np.arange(BIG_D) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    arg = t[:, None] * w[None, :]                            # float32 x float32 -> float32, rounded once
    assert arg.dtype == np.float32 and np.abs(arg).max() == 2.0 ** 30 and arg.min() < -2.0 ** 28
    dout = rng.standard_normal((BIG_N, BIG_D)).astype(np.float32)
    a64, d64, t64 = torch.from_numpy(arg).double(), torch.from_numpy(dout).double(), torch.from_numpy(t).double()
    g = -torch.sin(a64) * d64
    return dict(inputs=(torch.from_numpy(t), torch.from_numpy(w).view(BIG_D, 1), torch.zeros(BIG_D)),
                dout=torch.from_numpy(dout), arg=torch.from_numpy(arg), out=torch.cos(a64),
                grads=[(g * t64.view(-1, 1)).sum(0).view(BIG_D, 1), g.sum(0)])


def time_embedding_ref(x, rel_t, w, b):
    return x * (1 + (rel_t.view(-1, 1) * w.view(1, -1) + b.view(1, -1)))      # emb_module.py:48-50


@functools.lru_cache(maxsize=None)
def time_embedding_case(n, D):
    """rel_t = last_update - t <= 0 at JODIE's scale after normalising; w, b ~ N(0, 1) (TimeEmbedding's init)."""
    g = torch.Generator().manual_seed(n * 13 + D)
    x, rel_t = torch.randn(n, D, generator=g), -torch.rand(n, generator=g) * 50.0
    w, b = torch.randn(D, 1, generator=g), torch.randn(D, generator=g)
    dout = torch.randn(n, D, generator=g)
    inputs = (x, rel_t, w, b)
    out, grads = run_ref(time_embedding_ref, inputs, dout, torch.float64)
    return dict(inputs=inputs, dout=dout, out=out, grads=[grads[0], grads[2], grads[3]])


# ------------------------------------------------------------------ aggregators
AGG_DIMS = (1, 63, 64, 65, 129)
AGG_T_KINDS = ("long", "float")


@functools.lru_cache(maxsize=None)
def agg_case(dim, t_kind):
    """Rows at the wave boundary (a wave's lanes each take every 64th message of a row, then the lanes' firsts are
    merged by shuffles).  Message order inside a row is the order of the positions; the rows are interleaved.

      row 0 / 1 / 2   63 / 64 / 65 messages with one t: the first must win
      row 3           65 messages, the unique maximum is the 65th (lane 0's second pass)
      row 4           65 messages, the maximum ties between the 1st and the 65th (lane 0, both passes)
      row 5           no message
      row 6           70 messages with random t from a small range: many ties
      row 7 / 8       float: t = [-0.0, 0.0, -0.0] / [0.0, -0.0] — they tie (scatter_max), the first wins;
                      long: [-1, -1, -3] / [-5, -2]
    long t is negative throughout; float t is negative but for rows 7 / 8."""
    rng = np.random.default_rng(dim * 2 + (t_kind == "float"))
    rows = [np.full(63, -7.0), np.full(64, -9.0), np.full(65, -3.0),
            np.concatenate([rng.integers(-40, -10, 64), [-2]]).astype(np.float64),
            np.concatenate([[-4], rng.integers(-40, -10, 63), [-4]]).astype(np.float64),
            np.zeros(0), rng.integers(-6, -1, 70).astype(np.float64)]
    rows += [np.array([-0.0, 0.0, -0.0]), np.array([0.0, -0.0])] if t_kind == "float" else \
        [np.array([-1.0, -1.0, -3.0]), np.array([-5.0, -2.0])]
    dim_size = len(rows) + 1                                 # one more row without messages at the end
    label = rng.permutation(np.repeat(np.arange(len(rows)), [len(r) for r in rows]))
    t = np.zeros(label.shape[0])
    for r, vals in enumerate(rows):
        t[label == r] = vals                                 # in position order: the row's message order
    index = torch.from_numpy(label)
    tt = torch.from_numpy(t.astype(np.float32)) if t_kind == "float" else torch.from_numpy(t.astype(np.int64))
    if t_kind == "float":
        assert bool(torch.signbit(tt[index == 7][0])) and not bool(torch.signbit(tt[index == 7][1]))
    g = torch.Generator().manual_seed(dim)
    msg, dout = torch.randn(label.shape[0], dim, generator=g), torch.randn(dim_size, dim, generator=g)
    first = lambda r: int(torch.nonzero(index == r)[0])  # noqa: E731
    nth = lambda r, j: int(torch.nonzero(index == r)[j])  # noqa: E731
    expect_arg = {0: first(0), 1: first(1), 2: first(2), 3: nth(3, 64), 4: first(4), 5: label.shape[0],
                  7: first(7), 8: first(8) if t_kind == "float" else nth(8, 1)}
    return dict(msg=msg, index=index, t=tt, dim_size=dim_size, dout=dout, expect_arg=expect_arg)
