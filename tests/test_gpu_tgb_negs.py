"""GPU tests of the device pair index and the hist_rnd evaluation-negative generator (csrc/tgnx_negs.hip through
tgnx.tgb_negs and torch.ops.tgnx) against the numpy restatement tests/tgb_negs_ref.py: rows, k_hist and status equal
exactly.  tests/test_tgb_negs_cpu.py asserts which paths each stream takes (take-all / drawn historical part, sources
without history, several same-time positives, cyclic fill, empty valid set, many draw chunks, forced fill-up)."""
import numpy as np
import pytest
import torch

import tgb_negs_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, t=None, dtype=torch.float64):
    dev = torch.device("cuda")
    src, dst = torch.tensor(a["src"], device=dev), torch.tensor(a["dst"], device=dev)
    tt = torch.tensor(np.asarray(a["t"] if t is None else t), device=dev).to(dtype)
    return src, dst, tt, torch.tensor(a["pool"], device=dev)


def _raw(a, lo=None, hi=None, t=None, k=None, max_draws=0, index=None):
    """The ABI call on shape arguments `a`, nothing raised on status: (rows, k_hist, status) as numpy."""
    from tgnx.tgb_negs import PairHistory, hist_rnd
    src, dst, tt, pool = _dev(a, t)
    idx = index or PairHistory.build(src, dst, a["num_nodes"])
    lo, hi = a["lo"] if lo is None else lo, a["hi"] if hi is None else hi
    out = hist_rnd(src, dst, tt, lo, hi, a["k"] if k is None else k, a["q"], a["hist_hi"], pool, idx, seed=a["seed"],
                   max_draws=max_draws)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def _assert_equal(got, want, what):
    rows, kh, st = got
    assert np.array_equal(st, want[2]), (what, st, want[2])
    assert np.array_equal(kh, want[1]), (what, np.flatnonzero(kh != want[1])[:5])
    bad = np.flatnonzero((rows != want[0]).any(1))
    assert bad.size == 0, (what, bad[:5], rows[bad[:1]], want[0][bad[:1]])
    assert kh.dtype == np.int32 and rows.dtype == np.int64 and st.dtype == np.int64


@pytest.mark.parametrize("name", ["A", "B2", "B", "C", "D"])
def test_device_equals_restatement(name):
    a, want = R.case(name)
    _assert_equal(_raw(a), want, name)


def test_forced_fill_up_equals_restatement():
    a, want = R.case("A", 8)
    assert want[2][1] > 0 and want[2][2] > 0
    _assert_equal(_raw(a, max_draws=8), want, "A max_draws=8")


def test_halves_time_shift_and_float32():
    """Two half-range calls (history still cut at lo) and float64 stamps shifted to Unix-second magnitude give the
    one-call rows; the same shifted stamps as float32 merge and give the restatement's rows for the merged stamps."""
    a, want = R.case("A")
    lo, hi = a["lo"], a["hi"]
    mid = (lo + hi) // 2
    h0, h1 = _raw(a, lo, mid), _raw(a, mid, hi)
    assert np.array_equal(np.concatenate([h0[0], h1[0]]), want[0])
    assert np.array_equal(np.concatenate([h0[1], h1[1]]), want[1])
    _assert_equal(_raw(a, t=1.6e9 + a["t"]), want, "shifted float64")
    from tgnx.tgb_negs import PairHistory, hist_rnd
    src, dst, t32, pool = _dev(a, 1.6e9 + a["t"], torch.float32)
    got = hist_rnd(src, dst, t32, lo, hi, a["k"], a["q"], lo, pool, PairHistory.build(src, dst, a["num_nodes"]), seed=a["seed"])
    w32 = R.hist_rnd(a["src"], a["dst"], (1.6e9 + a["t"]).astype(np.float32), lo, hi, a["k"], a["q"], lo, a["pool"], a["seed"])
    _assert_equal(tuple(x.cpu().numpy() for x in got), w32, "shifted float32")
    assert not np.array_equal(w32[0], want[0])


def test_python_call_and_torch_op():
    """tgb_negatives (defaults: pool = unique(dst), hist_hi = lo, index built inside, q = int(k * hist_ratio)) and the
    torch op give the restatement's rows; an empty valid set raises ValueError naming the restatement's row."""
    from tgnx import ops
    from tgnx.tgb_negs import tgb_negatives
    a, want = R.case("A")
    src, dst, tt, pool = _dev(a)
    rows, kh, st = tgb_negatives(src, dst, tt, a["lo"], a["hi"], a["k"], seed=a["seed"], return_info=True)
    assert np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(kh.cpu().numpy(), want[1]) and st == [-1, 0, 0, 0]
    assert rows.is_cuda and tuple(rows.shape) == (a["hi"] - a["lo"], a["k"])
    rows_np = tgb_negatives(*(np.array(a[x]) for x in ("src", "dst", "t")), a["lo"], a["hi"], a["k"], seed=a["seed"])   # host arrays in
    assert np.array_equal(rows_np.cpu().numpy(), want[0])
    ns = ops.load()
    idx = ns.pair_index_build(src, dst, a["num_nodes"])
    o = ns.negs_hist_rnd(src, dst, tt, a["lo"], a["hi"], a["k"], a["q"], a["lo"], idx[0], idx[1], idx[2], pool, a["seed"], 0)
    _assert_equal(tuple(x.cpu().numpy() for x in o), want, "torch op")
    b, wb = R.case("B")
    assert wb[2][0] == 2
    src, dst, tt, pool = _dev(b)
    with pytest.raises(ValueError, match=rf"event row {b['lo'] + 2} \(output row 2\)"):
        tgb_negatives(src, dst, tt, b["lo"], b["hi"], b["k"], seed=b["seed"])
    with pytest.raises(ValueError, match="chronological"):
        tgb_negatives(src, dst, tt.flip(0), b["lo"], b["hi"], b["k"])


def test_k_above_1024_is_refused_without_a_launch():
    from tgnx import _lib
    a, _ = R.case("A")
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 1024\]"):
        _raw(a, k=1025)
    from tgnx.tgb_negs import tgb_negatives
    with pytest.raises(ValueError):
        tgb_negatives(np.array(a["src"]), np.array(a["dst"]), np.array(a["t"]), a["lo"], a["hi"], 1025)
    # the C entry point refuses before it touches a pointer: null everywhere, no device work
    rc = _lib.lib().tgnx_negs_hist_rnd(0, 0, 0, 1, 600, 420, 516, 1025, 512, 420, 0, 0, 0, 128, 0, 0, 80, 7, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"k must be in [1, 1024]" in _lib.lib().tgnx_last_error()


@pytest.mark.parametrize("name", ["A", "C"])
def test_pair_history_equals_numpy(name):
    from tgnx.tgb_negs import PairHistory
    a, _ = R.case(name)
    src, dst, _, _ = _dev(a)
    idx = PairHistory.build(src, dst, a["num_nodes"])
    indptr, indices, first = R.pair_index(a["src"], a["dst"], a["num_nodes"])
    assert np.array_equal(idx.indptr.cpu().numpy(), indptr)
    assert np.array_equal(idx.indices.cpu().numpy(), indices)
    assert np.array_equal(idx.first.cpu().numpy(), first)
    assert idx.nnz == indices.size and idx.num_rows == a["src"].size
    auto = PairHistory.build(np.array(a["src"]), np.array(a["dst"]))     # host arrays, num_nodes from the ids
    assert np.array_equal(auto.indices.cpu().numpy(), indices)


def test_contains_scalar_and_per_row_cut():
    """Queries: every pair of the stream at its own first row (not contained at that cut, contained one row later),
    random pairs, sources with an empty row and a source outside the index; scalar, per-row and absent cuts against
    the brute-force answer."""
    from tgnx.tgb_negs import PairHistory
    a, _ = R.case("A")
    src, dst, N = np.array(a["src"]), np.array(a["dst"]), a["num_nodes"]
    idx = PairHistory.build(src, dst, N)
    index = R.pair_index(src, dst, N)
    rng = np.random.default_rng(11)
    empty = [s for s in range(N) if index[0][s] == index[0][s + 1]]
    assert len(empty) >= 80                                             # (the destination ids never act as sources)
    qs = np.concatenate([src, rng.integers(0, 48, 500), np.array(empty[:20] + [N + 5, -1])])
    qd = np.concatenate([dst, rng.integers(48, 128, 500), rng.integers(48, 128, 22)])
    firsts = {}
    for j, (s, d) in enumerate(zip(src.tolist(), dst.tolist())):
        firsts.setdefault((s, d), j)
    f = np.array([firsts.get((int(s), int(d)), np.iinfo(np.int64).max) for s, d in zip(qs, qd)])
    exact = np.concatenate([np.array([firsts[(int(s), int(d))] for s, d in zip(src, dst)]),
                            rng.integers(0, 600, qs.size - src.size)])
    assert np.array_equal(idx.contains(qs, qd).cpu().numpy(), f < np.iinfo(np.int64).max)
    assert np.array_equal(idx.contains(qs, qd, before=300).cpu().numpy(), f < 300)
    at = idx.contains(qs, qd, before=torch.tensor(exact)).cpu().numpy()
    assert np.array_equal(at, f < exact) and not at[:src.size].any()    # first seen exactly at the cut: not contained
    after = idx.contains(qs, qd, before=exact + 1).cpu().numpy()
    assert np.array_equal(after, f < exact + 1) and after[:src.size].all()
    assert np.array_equal(R.contains(index, qs, qd, before=exact), at)
    got = idx.contains(qs, qd, before=exact)
    assert got.dtype == torch.bool and got.is_cuda


def test_bad_ids_are_refused():
    from tgnx.tgb_negs import PairHistory
    a, _ = R.case("A")
    bad = a["dst"].copy()
    bad[17] = 1 << 32
    with pytest.raises(RuntimeError, match="outside"):
        PairHistory.build(np.array(a["src"]), bad, a["num_nodes"])
    with pytest.raises(RuntimeError, match="outside"):
        PairHistory.build(np.array(a["dst"]), np.array(a["src"]), 48)   # sources >= num_nodes
    with pytest.raises(ValueError, match="2\\^32"):
        PairHistory.build(np.array(a["src"]), np.array(a["dst"]), (1 << 32) + 1)     # before anything is allocated
