"""The MFMA GEMM core (csrc/tgnx_gemm.h) on every tile config the library compiles, through the test hooks
tgnx_gemm_probe / tgnx_gemm_probe_batch (include/tgnx.h): G32 and G32L (16x16 wave split-K tiles, direct
operands, 2 / 3 slabs per round), GW (32x32, register-layout split-K partials), G64 (64x64) and GD (the public
entry's config), each direct and deferred (split-K + fixup launch), in all four transpose modes.

EXACT tests: operands, bias and the initial C are integers in [-3, 3] held in fp32, so every product and every
partial sum, in any order, is an integer below 2^24 (9 K + 6 < 2^24) and the result must torch.equal an int64
matmul on the CPU whatever the tile, split or wave order.  Every such run
  * fills the workspace with NaN (a partial that is read must have been written),
  * lays A, B and C in wider buffers (ld > logical width, slack words in front, two rows behind): operand
    padding is NaN, and so is every operand element past the RUNTIME sizes; C's padding holds a sentinel and a C
    that is not accumulated into starts as NaN,
  * checks that the Mr x Nr block is exact (so: NaN-free, every element written) and that every other word of
    C's buffer is bit-for-bit what it was,
  * runs twice from the same state and checks the two C buffers are bit-identical.
The sizes are the smallest at which a mechanism changes behaviour: ragged 16 / 32 / 64 tiles on either side of
the tile edge, K around the 16-B load rule (K % 4), the 16-deep slab, the 64-deep chunk and one vs two load rounds
(128 k at 2 slabs per round, 192 at 3), split counts below / at / above the chunk count, grid caps that make
workgroups loop, device-side runtime sizes (incl. Kr = 0: bias (+ C) exactly, Mr = 0: C untouched), a gathered A
operand, and operands whose base or leading dimension rules out 16-B loads (for the wave-split configs that
staged path must be bit-identical to the direct-operand path on random floats, as tgnx_gemm.h states).

FLOAT tests: randn operands against a float64 CPU product at the tolerance of test_gpu_gemm.py
(rtol 1e-5 sqrt(K) + 1e-6, atol 4 rtol).

BATCH hook: a direct G32 GEMM, two deferred GW GEMMs and a run of plain blocks in one gemmN launch, then one fixup
launch with head / tail blocks: all three products exact and every plain block ran exactly once.

One op-level case: link_predictor at the validation pass's shape class (16 800 candidate rows: hd and dz_dst on
G64, dW_dst on GD split 16 ways), forward and all eight gradients against the CPU oracle."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAN = float("nan")
SENTINEL = -12345.0
MODES = [(0, 1), (0, 0), (1, 1), (1, 0)]                      # (trans_a, trans_b)
CFGS = ["G32", "G32L", "GW", "G64", "GD"]
WAVE_SPLIT = ["G32", "G32L", "GD"]                            # direct-operand configs (16-B operands skip the LDS staging)
# M paired with two N each, on either side of the config's tile edge
PAIRS16 = [(1, 17), (1, 33), (15, 16), (15, 1), (16, 15), (16, 33), (17, 1), (17, 17), (33, 16), (33, 15)]
PAIRS32 = [(31, 32), (31, 65), (32, 33), (32, 31), (33, 65), (33, 32), (65, 31), (65, 33)]
PAIRS64 = [(63, 64), (63, 130), (64, 65), (64, 63), (65, 130), (65, 64), (130, 63), (130, 65)]
PAIRS = {"G32": PAIRS16, "G32L": PAIRS16, "GD": PAIRS16, "GW": PAIRS32, "G64": PAIRS64}
K_DIRECT = [1, 3, 4, 12, 16, 20, 60, 64, 68, 100, 128, 132, 192, 196, 252, 256]
K_SPLIT = [(64, 4), (65, 1), (130, 2), (260, 16), (448, 3), (572, 16), (1156, 16)]


def _L():
    from tgnx import _lib
    return _lib


class _Buf:
    """A logical rows x cols fp32 matrix inside a wider device buffer: `off` floats of slack in front, leading
    dimension ld >= cols, two more rows behind; everything outside the matrix holds `fill`."""

    def __init__(self, mat, ld, off, fill):
        rows, cols = mat.shape
        assert ld >= cols
        # 4 floats of slack behind `off` so that the (rows + 2) x ld extent always lies inside the allocation
        host = torch.full((off + (rows + 2) * ld + 4,), fill, dtype=torch.float32)
        host[off:off + rows * ld].view(rows, ld)[:, :cols] = mat
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.flat = host.to(DEV)
        self.init = host

    def ptr(self):
        return ctypes.c_void_p(self.flat.data_ptr() + 4 * self.off)

    def mat(self):
        return self.flat[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols].cpu()


def _bits(t):
    return t.cpu().view(torch.int32)


class _Case:
    """One GEMM problem (host data) and the launches over it."""

    def __init__(self, cfg, M, N, K, ta, tb, *, smax=0, cap=0, dims=None, bias=True, acc=False, gather=False,
                 kind="int"):
        self.cfg, self.M, self.N, self.K, self.ta, self.tb = cfg, M, N, K, ta, tb
        self.smax, self.cap, self.dims, self.acc, self.gather = smax, cap, dims, acc, gather
        g = torch.Generator().manual_seed(M * 7919 + N * 104729 + K * 31 + ta * 2 + tb)

        def draw(*shape):
            if kind == "int":
                return torch.randint(-3, 4, shape, generator=g).float()
            return torch.randn(*shape, generator=g)
        self.H = M + 9 if gather else M                       # rows of the stored A that a_rows picks from
        self.A = draw(K, M) if ta else draw(self.H, K)
        self.B = draw(N, K) if tb else draw(K, N)
        self.bias = draw(N) if bias else None
        self.C0 = draw(M, N)
        # a permutation of A's rows with repeats (row 0 of A three times)
        self.rows = None
        if gather:
            self.rows = torch.randperm(self.H, generator=g)[:M].clone()
            self.rows[M // 2] = self.rows[0]
            self.rows[M - 1] = self.rows[0]
        Mr, Nr, Kr = M, N, K
        if dims is not None:
            Mr, Nr, Kr = (c if d < 0 else d for d, c in zip(dims, (M, N, K)))
        self.Mr, self.Nr, self.Kr = Mr, Nr, Kr

    def op_a(self):
        a = self.A.t() if self.ta else (self.A[self.rows] if self.gather else self.A)
        return a[:self.Mr, :self.Kr]

    def op_b(self):
        b = self.B.t() if self.tb else self.B
        return b[:self.Kr, :self.Nr]

    def expected(self, dtype=torch.int64):
        """The Mr x Nr block: the product over the first Kr of k, plus the epilogue."""
        e = self.op_a().to(dtype) @ self.op_b().to(dtype)
        if self.bias is not None:
            e = e + self.bias[:self.Nr].to(dtype)
        if self.acc:
            e = e + self.C0[:self.Mr, :self.Nr].to(dtype)
        return e

    def launch(self, *, a_off=4, b_off=4, lda_pad=4, ldb_pad=4, ldc_pad=3):
        """Run once from the initial state; returns C's _Buf.  The allocations are 16-B aligned (torch: 256 B)
        and the operand starts `off` floats in: off = 4 and ld = width + 4 keep a k-contiguous operand with
        K % 4 == 0 eligible for 16-B loads, an off that is no multiple of 4 or an odd ld pad rule them out."""
        L = _L()
        A, B = self.A.clone(), self.B.clone()
        if self.dims is not None:                             # operand elements past the runtime sizes: NaN
            if self.ta:
                A[self.Kr:, :], A[:, self.Mr:] = NAN, NAN
            else:
                A[:, self.Kr:] = NAN
                if not self.gather:
                    A[self.Mr:, :] = NAN
            if self.tb:
                B[self.Nr:, :], B[:, self.Kr:] = NAN, NAN
            else:
                B[self.Kr:, :], B[:, self.Nr:] = NAN, NAN
        a = _Buf(A, A.shape[1] + lda_pad, a_off, NAN)
        b = _Buf(B, B.shape[1] + ldb_pad, b_off, NAN)
        c0 = self.C0 if self.acc else torch.full((self.M, self.N), NAN)
        c = _Buf(c0, self.N + ldc_pad, 1, SENTINEL)
        bias = self.bias.to(DEV) if self.bias is not None else None
        rows = self.rows.to(DEV) if self.gather else None
        dims = torch.tensor(self.dims, dtype=torch.int32, device=DEV) if self.dims is not None else None
        ci = L.GEMM_PROBE_CFGS[self.cfg]
        nb = L.lib().tgnx_gemm_probe_ws_bytes(ci, self.smax, self.M, self.N, self.K)
        assert nb % 4 == 0
        ws = torch.full((nb // 4,), NAN, dtype=torch.float32, device=DEV)
        L.call("tgnx_gemm_probe", ci, self.smax, self.cap, self.M, self.N, self.K, L.ptr(dims), a.ptr(), a.ld,
               self.ta, L.ptr(rows), b.ptr(), b.ld, self.tb, c.ptr(), c.ld, L.ptr(bias), int(self.acc), L.ptr(ws),
               ctypes.c_size_t(nb), L.stream())
        torch.cuda.synchronize()
        return c

    def check_exact(self, what="", **kw):
        c = self.launch(**kw)
        got = c.mat()[:self.Mr, :self.Nr]
        want = self.expected().float()
        tag = (what, self.cfg, self.M, self.N, self.K, self.ta, self.tb, self.smax, self.cap, self.dims, kw)
        if not torch.equal(got, want):
            bad = (got != want) | got.isnan()
            idx = bad.nonzero()[:8].tolist()
            raise AssertionError(f"{tag}: {int(bad.sum())} wrong elements, first at {idx}: "
                                 f"got {[float(got[i, j]) for i, j in idx]} want {[float(want[i, j]) for i, j in idx]}")
        # every word outside the block is what it was: C's padding (sentinel) and, with runtime sizes, the rest of C
        after, before = _bits(c.flat), _bits(c.init)
        blk = torch.zeros(c.init.shape, dtype=torch.bool)
        blk[c.off:c.off + c.rows * c.ld].view(c.rows, c.ld)[:self.Mr, :self.Nr] = True
        assert torch.equal(after[~blk], before[~blk]), (tag, "C written outside its Mr x Nr block")
        c2 = self.launch(**kw)
        assert torch.equal(_bits(c2.flat), after), (tag, "second run differs")
        return c


ALIGNED = dict(a_off=4, b_off=4, lda_pad=4, ldb_pad=4)        # 16-B loads where K % 4 == 0 and the operand is k-fast


# ------------------------------------------------------------------ exact: direct and deferred, every config
@pytest.mark.parametrize("ta,tb", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_exact_direct(cfg, ta, tb):
    for K, (M, N) in itertools.product(K_DIRECT, PAIRS[cfg]):
        _Case(cfg, M, N, K, ta, tb).check_exact("direct", **ALIGNED)


@pytest.mark.parametrize("ta,tb", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_exact_deferred(cfg, ta, tb):
    for (K, smax), (M, N) in itertools.product(K_SPLIT, PAIRS[cfg]):
        _Case(cfg, M, N, K, ta, tb, smax=smax).check_exact("deferred", **ALIGNED)


# ------------------------------------------------------------------ grid cap: workgroups loop over the tiles past it
@pytest.mark.parametrize("cap", [8, 16])
@pytest.mark.parametrize("cfg,M,N,K,smax", [("G32", 70, 50, 130, 3),     # 5 x 4 tiles x 3 splits = 60 workgroups uncapped
                                            ("G32", 70, 50, 130, 0),     # 20 tiles, direct
                                            ("G32L", 70, 50, 132, 0),
                                            ("GW", 70, 50, 260, 4),      # 3 x 2 tiles x 4 splits = 24
                                            ("G64", 130, 200, 260, 5),   # 3 x 4 tiles x 5 splits = 60
                                            ("GD", 70, 50, 572, 16)])    # 20 tiles x 9 splits = 180
def test_exact_grid_cap(cfg, M, N, K, smax, cap):
    for ta, tb in MODES:
        _Case(cfg, M, N, K, ta, tb, smax=smax, cap=cap, acc=True).check_exact("cap", **ALIGNED)


# ------------------------------------------------------------------ device-side runtime sizes below the capacity
DIMS = [(70, 50, 300), (17, 50, 300), (1, 50, 300), (70, 33, 300), (70, 50, 0), (70, 50, 3), (70, 50, 64),
        (70, 50, 260), (0, 50, 300),
        (-1, 33, -1), (17, -1, 3), (-1, -1, 0)]              # (an entry < 0: that size is not passed)


@pytest.mark.parametrize("ta,tb", MODES)
@pytest.mark.parametrize("cfg,smax", [("G32", 0), ("GW", 4), ("G32L", 16), ("G64", 0), ("G64", 4)])
def test_exact_runtime_dims(cfg, smax, ta, tb):
    for dims, (bias, acc) in itertools.product(DIMS, [(True, False), (True, True)]):
        _Case(cfg, 70, 50, 300, ta, tb, smax=smax, dims=dims, bias=bias, acc=acc).check_exact("dims", **ALIGNED)


def test_runtime_k_zero_and_m_zero_leave_what_they_must():
    """Kr = 0 (the first batch of an epoch: no edges yet): C = bias (+ C0) exactly, never a stale partial; Mr = 0:
    not one word of C changes.  (check_exact covers both; this states them on their own.)"""
    for cfg, smax in [("G32", 0), ("GW", 4), ("G64", 4), ("GD", 16)]:
        for acc in (False, True):
            case = _Case(cfg, 70, 50, 300, 1, 0, smax=smax, dims=(70, 50, 0), acc=acc)
            got = case.check_exact("Kr=0", **ALIGNED).mat()
            want = case.bias.expand(70, 50) + (case.C0 if acc else 0)
            assert torch.equal(got, want)
            case = _Case(cfg, 70, 50, 300, 1, 0, smax=smax, dims=(0, 50, 300), acc=acc)
            c = case.check_exact("Mr=0", **ALIGNED)
            assert torch.equal(_bits(c.flat), _bits(c.init))


# ------------------------------------------------------------------ gathered A (two-phase loader)
@pytest.mark.parametrize("cfg,smax,K", [("G32L", 0, 100), ("G32L", 0, 196), ("GW", 4, 260), ("GD", 0, 5),
                                        ("G32", 0, 132), ("G64", 3, 260), ("GD", 16, 572)])
def test_exact_gather(cfg, smax, K):
    for tb, (M, N) in itertools.product((1, 0), PAIRS[cfg][::2]):
        _Case(cfg, M, N, K, 0, tb, smax=smax, gather=True).check_exact("gather", **ALIGNED)
        # a leading dimension that rules out 16-B loads: the element-wise gather path
        _Case(cfg, M, N, K, 0, tb, smax=smax, gather=True).check_exact("gather", a_off=4, b_off=4, lda_pad=5,
                                                                       ldb_pad=4)
    # runtime sizes below the gather's capacity
    _Case(cfg, 70, 50, K, 0, 1, smax=smax, gather=True, dims=(17, 33, K - (K > 4))).check_exact("gather", **ALIGNED)


# ------------------------------------------------------------------ operands that rule out 16-B loads
MISALIGNED = [dict(a_off=1, b_off=4, lda_pad=4, ldb_pad=4), dict(a_off=4, b_off=1, lda_pad=4, ldb_pad=4),
              dict(a_off=4, b_off=4, lda_pad=5, ldb_pad=4), dict(a_off=4, b_off=4, lda_pad=4, ldb_pad=5),
              dict(a_off=3, b_off=2, lda_pad=5, ldb_pad=9)]


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_misaligned_operands(cfg):
    M, N = PAIRS[cfg][5]
    for (K, smax), (ta, tb), lay in itertools.product([(60, 0), (132, 0), (196, 0), (260, 16)], MODES, MISALIGNED):
        _Case(cfg, M, N, K, ta, tb, smax=smax).check_exact("misaligned", **lay)


@pytest.mark.parametrize("cfg", WAVE_SPLIT)
def test_staged_path_bit_identical_to_direct_operands(cfg):
    """tgnx_gemm.h, gemm_tile_direct: 'the same slabs, k order, accumulator chains and wave-order combine as the
    LDS-staged WS path, so the results are bit-identical to it'.  16-B-aligned operands take the direct-operand
    path, the same data one float off (or with ld % 4 == 1) the staged one: random floats, compared bit for bit."""
    for (M, N, K, smax), (ta, tb) in itertools.product([(33, 17, 196, 0), (70, 50, 572, 0), (70, 50, 572, 16),
                                                        (17, 33, 1156, 3)], MODES):
        case = _Case(cfg, M, N, K, ta, tb, smax=smax, kind="randn")
        ref = case.launch(**ALIGNED).mat()
        assert not ref.isnan().any()
        for lay in MISALIGNED:
            assert torch.equal(_bits(case.launch(**lay).mat()), _bits(ref)), (cfg, M, N, K, smax, ta, tb, lay)


# ------------------------------------------------------------------ epilogue: bias x accumulate
@pytest.mark.parametrize("bias,acc", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("cfg", CFGS)
def test_exact_epilogue(cfg, bias, acc):
    M, N = PAIRS[cfg][4]
    for (K, smax), (ta, tb) in itertools.product([(100, 0), (260, 4)], MODES):
        _Case(cfg, M, N, K, ta, tb, smax=smax, bias=bias, acc=acc).check_exact("epilogue", **ALIGNED)


# ------------------------------------------------------------------ argument checks: an error code, no launch
def test_probe_rejects_bad_arguments():
    L = _L()
    lib = L.lib()
    M, N, K = 33, 17, 260
    A, B = torch.zeros(M, K, device=DEV), torch.zeros(N, K, device=DEV)
    C = torch.full((M, N), SENTINEL, device=DEV)
    rows = torch.zeros(M, dtype=torch.int64, device=DEV)
    gw = L.GEMM_PROBE_CFGS["GW"]
    nb = lib.tgnx_gemm_probe_ws_bytes(gw, 4, M, N, K)
    assert nb > 256                                           # split partials
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)

    def rc(cfg=gw, smax=4, ta=0, a_rows=None, nbytes=nb, lda=K):
        return lib.tgnx_gemm_probe(cfg, smax, 0, M, N, K, None, L.ptr(A), lda, ta, L.ptr(a_rows), L.ptr(B), K, 1,
                                   L.ptr(C), N, None, 0, L.ptr(ws), ctypes.c_size_t(nbytes), L.stream())
    assert rc(nbytes=nb - 1) != 0 and b"workspace" in lib.tgnx_last_error()
    assert rc(ta=1, a_rows=rows, lda=M) != 0 and b"a_rows" in lib.tgnx_last_error()
    assert rc(cfg=5) != 0 and b"cfg" in lib.tgnx_last_error()
    assert rc(cfg=-1) != 0
    assert rc(lda=K - 1) != 0
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())                        # nothing ran
    assert rc() == 0                                          # and the same call with good arguments does
    torch.cuda.synchronize()
    assert bool((C == 0).all())


# ------------------------------------------------------------------ float: randn against float64
@pytest.mark.parametrize("cfg,M,N,K,smax", [(c, 413, 400, 572, s) for c in WAVE_SPLIT for s in (0, 16)] +
                         [("GW", 100, 573, 415, 0), ("GW", 100, 573, 415, 3),
                          ("G64", 130, 200, 260, 0), ("G64", 130, 200, 260, 16)])
def test_float_matches_float64(cfg, M, N, K, smax):
    tol = 1e-5 * (K ** 0.5) + 1e-6                            # tests/test_gpu_gemm.py
    for ta, tb in MODES:
        case = _Case(cfg, M, N, K, ta, tb, smax=smax, kind="randn")
        got = case.launch(**ALIGNED).mat()
        ref = case.expected(torch.float64)
        err = (got.double() - ref).abs()
        print(f"{cfg} {M}x{N}x{K} smax {smax} ta {ta} tb {tb}: max err {float(err.max()):.3e} "
              f"(rtol {tol:.3e}, atol {4 * tol:.3e})")
        assert torch.allclose(got, ref.float(), rtol=tol, atol=4 * tol), float(err.max())


# ------------------------------------------------------------------ several jobs in one launch + one fixup launch
def _batch(head, tail_blocks, nb=11, expect_ok=True):
    L = _L()
    lib = L.lib()
    g = torch.Generator().manual_seed(17 + head * 3 + tail_blocks)

    def ints(*shape):
        return torch.randint(-3, 4, shape, generator=g).float()
    # (M, N, K, smax, A stored shape, B stored shape); jobs[1] is C = A^T B
    shapes = [(70, 50, 132, 0), (65, 33, 260, 4), (33, 100, 448, 3)]
    jobs = (L.GemmProbeJob * 3)()
    keep, want, cbufs = [], [], []
    for i, (M, N, K, smax) in enumerate(shapes):
        A = ints(K, M) if i == 1 else ints(M, K)
        B = ints(K, N) if i == 1 else ints(N, K)
        bias, C0 = ints(N), ints(M, N)
        acc = i != 1
        a, b = _Buf(A, A.shape[1] + 4, 4, NAN), _Buf(B, B.shape[1] + 4, 4, NAN)
        c = _Buf(C0 if acc else torch.full((M, N), NAN), N + 3, 1, SENTINEL)
        bd = bias.to(DEV)
        keep += [a, b, bd]
        cbufs.append(c)
        opa, opb = (A.t(), B) if i == 1 else (A, B.t())
        want.append((opa.long() @ opb.long() + bias.long() + (C0.long() if acc else 0)).float())
        jobs[i] = L.GemmProbeJob(M, N, K, a.ptr().value, a.ld, b.ptr().value, b.ld, c.ptr().value, c.ld,
                                 bd.data_ptr(), int(acc), smax)
    marks = torch.zeros(max(nb, 1), dtype=torch.int32, device=DEV)
    tail_marks = torch.zeros(max(tail_blocks, 1), dtype=torch.int32, device=DEV)
    nt = sum(-(-M // 32) * -(-N // 32) for M, N, _, _ in shapes[1:])      # GW: 32x32 output tiles
    fix_blocks = torch.full((nt,), -1, dtype=torch.int32, device=DEV)
    nbytes = lib.tgnx_gemm_probe_batch_ws_bytes(jobs)
    assert nbytes > 256 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), NAN, dtype=torch.float32, device=DEV)
    rc = lib.tgnx_gemm_probe_batch(jobs, nb, L.ptr(marks), head, tail_blocks, L.ptr(tail_marks),
                                   L.ptr(fix_blocks), L.ptr(ws), ctypes.c_size_t(nbytes), L.stream())
    torch.cuda.synchronize()
    if not expect_ok:
        assert rc != 0
        assert all(torch.equal(_bits(c.flat), _bits(c.init)) for c in cbufs)
        return None
    assert rc == 0, lib.tgnx_last_error()
    for i, (c, w) in enumerate(zip(cbufs, want)):
        assert torch.equal(c.mat(), w), (i, head, tail_blocks)
        blk = torch.zeros(c.init.shape, dtype=torch.bool)
        blk[c.off:c.off + c.rows * c.ld].view(c.rows, c.ld)[:, :c.cols] = True
        assert torch.equal(_bits(c.flat)[~blk], _bits(c.init)[~blk]), (i, "padding")
    assert marks.cpu().tolist() == [1] * nb + [0] * (max(nb, 1) - nb)
    assert tail_marks.cpu().tolist() == [1] * tail_blocks + [0] * (max(tail_blocks, 1) - tail_blocks)
    # tgnx_gemm.h, gemm_fixup_kernel: the fix range is padded to a multiple of the 8 XCDs and XCD x (the blocks
    # with bid % 8 == x past the head) takes the run [x nfix / 8, (x + 1) nfix / 8) of tiles in order
    per = -(-nt // 8)
    assert fix_blocks.cpu().tolist() == [head + 8 * (t % per) + t // per for t in range(nt)]
    return [_bits(c.flat) for c in cbufs]


@pytest.mark.parametrize("head,tail_blocks", [(0, 0), (0, 5), (3, 5), (5, 5)])
def test_batch_launch_runs_every_job_and_block_once(head, tail_blocks):
    first = _batch(head, tail_blocks)
    again = _batch(head, tail_blocks)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    _batch(head, tail_blocks, nb=0)                           # no plain blocks in the GEMM launch


def test_batch_rejects_head_past_tail_blocks():
    """`head` counts the tail blocks that lead the fixup grid, so head <= tail_blocks (gemm_fixup_kernel): with
    head = 3 of 0 tail blocks the grid would lose its last three fix tiles.  An error code, no launch."""
    _batch(3, 0, expect_ok=False)


# ------------------------------------------------------------------ link_predictor at the validation pass's shape class
def test_link_predictor_validation_shape_grads_match_oracle():
    """n_src = 24 sources x k = 700 candidates (the eval `tile` pairing): M = 16 800 rows, D = 100.  hd = z_dst
    W_dst^T and dz_dst run on G64 (263 x 2 = 526 tiles of 64x64), dW_dst on GD split 16 ways over 263 chunks.
    Tolerances and error measure of test_gpu_module_grads.py."""
    from oracle.tgnn_ref import RefEdgePredictor
    from tgnx.ops import link_predictor
    FWD_TOL, GRAD_TOL = 2e-5, 1e-4

    def close(a, b, tol, what):
        assert a.shape == b.shape, (what, a.shape, b.shape)
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        scale = max(float(b.abs().max()), 1.0)
        err = float((a - b).abs().max())
        print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e} tol {tol:g}")
        assert err <= tol * scale, (what, err, scale)
    n_src, k, D = 24, 700, 100
    M = n_src * k
    torch.manual_seed(n_src * 10 + k)
    zs, zd = torch.randn(n_src, D, requires_grad=True), torch.randn(M, D, requires_grad=True)
    dout = torch.randn(M, 1)
    ep = RefEdgePredictor(D, D)
    params = [ep.src_fc.weight, ep.src_fc.bias, ep.dst_fc.weight, ep.dst_fc.bias, ep.out_fc.weight, ep.out_fc.bias]
    _, want = ep(zs, zd[:n_src], zd, neg_samples=k)
    want.backward(dout)

    def run():
        leaves = [t.detach().to(DEV).requires_grad_(True) for t in [zs, zd] + params]
        out = link_predictor(*leaves, sigmoid=False)
        out.backward(dout.to(DEV))
        return out, leaves
    out, leaves = run()
    close(out, want, FWD_TOL, "pred out")
    names = ("z_src", "z_dst", "w_src", "b_src", "w_dst", "b_dst", "w_out", "b_out")
    for got, ref, n in zip(leaves, [zs, zd] + params, names):
        close(got.grad, ref.grad, GRAD_TOL, f"pred d{n} n_src={n_src} k={k}")
    out2, again = run()
    assert torch.equal(out, out2)
    for a, b in zip(leaves, again):
        assert torch.equal(a.grad, b.grad)
