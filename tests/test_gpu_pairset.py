"""GPU tests of the live pair set operator (csrc/tgnx_pairset.hip, tgnx/pairset.py, torch.ops.tgnx.pairset_*) against
the dict reference (tests/pairset_ref.py): exact equality everywhere, sets compared in the sorted form only.

  insert / lookup   N = 50; batches of 1, 64 and 200 events, one of them a single pair 200 times; self-pairs, ids 0 and
                    N - 1, equal stamps, stamps -1.0 / 0.0 / 1.6e9; an id = N and a NaN stamp counted and absent
  collisions        capacity 64: 24 keys of home slot 63 (found from the documented formula) wrap and are all present,
                    8 more of the same home slot are absent
  growth            1,000 distinct pairs in calls of 8 from capacity 64: contents, n_keys, load <= 1/2 after every call
  full table        the raw ABI call, 80 keys into capacity 64: returns, counts add up, nothing invented
  select            Q = 3 (no history / every candidate / mixed), C = 130 with a duplicate and a stranger, two cuts,
                    Q = 0 and C = 0, two runs bit-equal, several blocks per source at C = 2,100
  state / erase     round trip, erase_nodes, to_pair_history, the torch ops"""
import numpy as np
import pytest
import torch

import pairset_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 50


def _set(num_nodes=N, capacity=64):
    from tgnx.pairset import PairSet
    return PairSet(num_nodes, capacity, device=DEV)


def _assert_lookup(ps, ref, src, dst, since=None):
    got = ps.lookup(src, dst, since)
    want = ref.lookup(src, dst, since)
    for g, w, name in zip(got, want, ("seen", "count", "t_first", "t_last")):
        assert np.array_equal(g.cpu().numpy(), w), name
    assert np.array_equal(ps.contains(src, dst, since).cpu().numpy(), want[0])


def _grid(n=N):
    s, d = np.divmod(np.arange(n * n), n)
    return s, d


def test_insert_and_lookup_match_the_reference():
    rng = np.random.default_rng(0)
    ps, ref = _set(capacity=2048), R.RefPairSet(N)
    batches = [(np.array([7]), np.array([7]), np.array([5.0], np.float32)),                      # 1 event, a self-pair
               (rng.integers(0, N, 64), rng.integers(0, N, 64), np.sort(rng.random(64).astype(np.float32) * 100)),
               (np.full(200, 3), np.full(200, 9), rng.permutation(200).astype(np.float32) - 50),   # one pair 200 times
               (rng.integers(0, N, 200), rng.integers(0, N, 200), np.full(200, 77.0, np.float32)),  # equal stamps
               (np.array([0, N - 1, 0, N - 1, 0]), np.array([N - 1, 0, 0, N - 1, N - 1]),
                np.array([-1.0, 0.0, 1.6e9, -0.0, 1.6e9], np.float32))]
    for s, d, t in batches:
        ps.insert(s, d, t)
        ref.insert(s, d, t)
    assert ps.counters() == dict(n_keys=ref.n_keys, n_invalid=0, n_overflow=0)
    _assert_lookup(ps, ref, *_grid())
    seen, cnt, tf, tl = (x.cpu().numpy() for x in ps.lookup([3], [9]))
    assert seen[0] and cnt[0] == 200 and tf[0] == -50.0 and tl[0] == 149.0
    R.assert_state_equal(ps.state(), ref)
    # an id = N and a NaN stamp: counted, never inserted
    s, d, t = np.array([N, 1, 2, 4]), np.array([1, N, 2, 5]), np.array([1.0, 1.0, np.nan, 2.0], np.float32)
    ps.insert(s, d, t)
    ref.insert(s, d, t)
    assert ref.n_invalid == 3 and ps.counters() == dict(n_keys=ref.n_keys, n_invalid=3, n_overflow=0)
    _assert_lookup(ps, ref, np.array([N, 1, 2, 4, -1]), np.array([1, N, 2, 5, 0]))
    # cuts: one for all, one per query, on stamps the set holds
    for cut in (-1.0, 0.0, 77.0, 77.5, 1.6e9, float("inf")):
        _assert_lookup(ps, ref, *_grid(), since=cut)
    gs, gd = _grid()
    _assert_lookup(ps, ref, gs, gd, since=rng.choice(np.array([-2.0, 0.0, 50.0, 77.0, 2e9], np.float32), gs.size))


def test_collisions_wrap_and_absent_keys_of_the_same_home_slot():
    s, d = R.colliding_keys(64, 63, 32, N)
    assert (R.home_slot(R.pair_key(s, d), 64) == 63).all()
    ps, ref = _set(capacity=64), R.RefPairSet(N)
    t = np.arange(24, dtype=np.float32)
    for a in range(0, 24, 8):                                  # (capacity / 8 per call; 24 <= capacity / 2: no growth)
        ps.insert(s[a:a + 8], d[a:a + 8], t[a:a + 8])
        ref.insert(s[a:a + 8], d[a:a + 8], t[a:a + 8])
    assert ps.capacity == 64 and ps.counters() == dict(n_keys=24, n_invalid=0, n_overflow=0)
    _assert_lookup(ps, ref, s, d)
    assert ps.contains(s[:24], d[:24]).all() and not ps.contains(s[24:], d[24:]).any()
    R.assert_state_equal(ps.state(), ref)


def test_growth_from_capacity_64():
    rng = np.random.default_rng(1)
    pick = rng.permutation(N * N)[:1000]
    s, d = np.divmod(pick, N)
    t = rng.random(1000).astype(np.float32)
    ps, ref = _set(capacity=64), R.RefPairSet(N)
    caps = [64]
    for a in range(0, 1000, 8):
        ps.insert(s[a:a + 8], d[a:a + 8], t[a:a + 8])
        ref.insert(s[a:a + 8], d[a:a + 8], t[a:a + 8])
        c = ps.counters()
        assert c == dict(n_keys=ref.n_keys, n_invalid=0, n_overflow=0) and c["n_keys"] <= ps.capacity // 2
        if ps.capacity != caps[-1]:
            caps.append(ps.capacity)
    assert len(caps) > 2 and ps.n_keys == 1000
    assert ps.reads <= 1000 // 8                                # (scheduled reads, not one per call)
    R.assert_state_equal(ps.state(), ref)
    _assert_lookup(ps, ref, *_grid())


def test_full_table_returns_and_counts_the_overflow():
    from tgnx import _lib
    ps = _set(capacity=64)
    s, d = np.divmod(np.random.default_rng(2).permutation(N * N)[:80], N)
    src, dst = torch.from_numpy(s).to(DEV), torch.from_numpy(d).to(DEV)
    t = torch.arange(80, dtype=torch.float32, device=DEV)
    _lib.call("tgnx_pairset_insert", ps.table.data_ptr(), 64, src.data_ptr(), dst.data_ptr(), t.data_ptr(), 80, N,
              ps.status.data_ptr(), _lib.stream(DEV))          # the raw call: no growth rule
    c = ps.counters()
    assert c["n_keys"] <= 64 and c["n_overflow"] == 80 - c["n_keys"] and c["n_invalid"] == 0
    gs, gd = _grid()
    seen = ps.contains(gs, gd).cpu().numpy()
    assert int(seen.sum()) == c["n_keys"]
    assert set(zip(gs[seen].tolist(), gd[seen].tolist())) <= set(zip(s.tolist(), d.tolist()))
    st = ps.state()
    assert st["keys"].numel() == c["n_keys"] and bool((st["count"] == 1).all())


def _select_case(C=130):
    """Sources 5 (no history), 6 (met every candidate but the stranger), 7 (mixed); the candidates hold a duplicate and
    the stranger, node n - 1, which no event names.  Returns (set, reference, sources, candidates, a mid-stream cut)."""
    rng = np.random.default_rng(3)
    n = 3000
    cand = rng.permutation(n - 1)[:C].astype(np.int64)
    cand[17] = cand[3]                                         # a duplicate
    cand[40] = n - 1                                           # never inserted
    known = np.delete(cand, 40)
    ps, ref = _set(num_nodes=n, capacity=2 * _pow2(C + 600)), R.RefPairSet(n)
    ev_s = np.concatenate([np.full(C - 1, 6), np.full(C // 2, 7), rng.integers(8, n - 1, 200)])
    ev_d = np.concatenate([known, known[::2][:C // 2], rng.integers(0, n - 1, 200)])
    ev_t = np.arange(ev_s.size, dtype=np.float32)
    for a in range(0, ev_s.size, 128):
        sl = slice(a, a + 128)
        ps.insert(ev_s[sl], ev_d[sl], ev_t[sl])
        ref.insert(ev_s[sl], ev_d[sl], ev_t[sl])
    return ps, ref, np.array([5, 6, 7]), cand, float(ev_t[C - 1 + C // 4])


def _pow2(n):
    return 1 << (int(n) - 1).bit_length()


@pytest.mark.parametrize("C", [130, 2100])
def test_select_matches_the_reference(C):
    ps, ref, src, cand, mid = _select_case(C)
    for since in (None, mid, np.array([0.0, mid, 1e9], np.float32)):
        ptr, ids = ps.select(src, cand, since)
        wptr, wids = ref.select(src, cand, since)
        assert np.array_equal(ptr.cpu().numpy(), wptr) and np.array_equal(ids.cpu().numpy(), wids)
        ptr2, ids2 = ps.select(src, cand, since)
        assert torch.equal(ptr, ptr2) and torch.equal(ids, ids2)            # run to run, bit for bit
    ptr, ids = ps.select(src, cand)
    p = ptr.tolist()
    assert p[1] == 0 and p[2] - p[1] == C - 1 and 0 < p[3] - p[2] < C - 1   # none, all but the stranger, mixed
    assert (ids == 3000 - 1).sum() == 0 and (ids == int(cand[3])).sum() >= 2  # the stranger never, the duplicate twice
    ptr, ids = ps.select(src, np.delete(cand, 40))
    assert (ptr[2] - ptr[1]).item() == C - 1                                # every candidate met
    ptr, ids = ps.select(np.zeros(0, np.int64), cand)
    assert ptr.tolist() == [0] and ids.numel() == 0
    ptr, ids = ps.select(src, np.zeros(0, np.int64))
    assert ptr.tolist() == [0, 0, 0, 0] and ids.numel() == 0
    # ids out of range are never met, as sources or as candidates
    ptr, ids = ps.select(np.array([-1, 3000, 6]), np.array([-1, 3000, int(cand[0])]))
    assert ptr.tolist() == [0, 0, 0, 1] and ids.tolist() == [int(cand[0])]


def test_state_round_trip_erase_and_torch_ops():
    rng = np.random.default_rng(4)
    s, d, t = rng.integers(0, N, 400), rng.integers(0, N, 400), rng.random(400).astype(np.float32)
    ps, ref = _set(capacity=64), R.RefPairSet(N)
    for a in range(0, 400, 8):
        ps.insert(s[a:a + 8], d[a:a + 8], t[a:a + 8])
    ref.insert(s, d, t)
    st = ps.state()
    R.assert_state_equal(st, ref)
    assert bool((st["keys"][1:] > st["keys"][:-1]).all())
    other = _set(capacity=64)
    other.load_state({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()})
    R.assert_state_equal(other.state(), ref)
    assert other.n_keys == ref.n_keys <= other.capacity // 4
    _assert_lookup(other, ref, *_grid())
    other.insert(s[:8], d[:8], t[:8] + 5)                       # a loaded set goes on
    ref2 = R.RefPairSet(N)
    ref2.insert(np.concatenate([s, s[:8]]), np.concatenate([d, d[:8]]), np.concatenate([t, t[:8] + 5]))
    R.assert_state_equal(other.state(), ref2)
    bad = dict(st, keys=st["keys"].clone())
    bad["keys"][0] = (N << 32) | 1
    with pytest.raises(RuntimeError, match="load_state"):
        other.load_state(bad)
    R.assert_state_equal(other.state(), ref2)                   # a refused state leaves the set as it was
    other.insert(s[:8], d[:8], t[:8])                           # ... and usable
    ref2.insert(s[:8], d[:8], t[:8])
    R.assert_state_equal(other.state(), ref2)
    # the CSR form
    ph = ps.to_pair_history()
    keys = ref.sorted_state()[0]
    assert ph.first is None and ph.indices.tolist() == (keys & 0xFFFFFFFF).tolist()
    assert ph.indptr.tolist() == np.searchsorted(keys >> 32, np.arange(N + 1)).tolist()
    # erase
    busiest = int(np.bincount(np.concatenate([s, d]), minlength=N).argmax())
    gone = ps.erase_nodes([busiest, 0, 0])
    assert gone == ref.erase([busiest, 0]) and gone > 0 and ps.n_keys == ref.n_keys
    R.assert_state_equal(ps.state(), ref)
    _assert_lookup(ps, ref, *_grid())
    with pytest.raises(ValueError, match="node ids"):
        ps.erase_nodes([N])
    # the torch ops over the same table
    from tgnx import ops
    T = ops.load()
    gs, gd = (torch.from_numpy(x).to(DEV) for x in _grid())
    got = T.pairset_lookup(ps.table, gs, gd, N)
    for g, w in zip(got, ps.lookup(gs, gd)):
        assert torch.equal(g, w)
    assert torch.equal(T.pairset_lookup(ps.table, gs, gd, N, None, 0.5)[0], ps.contains(gs, gd, 0.5))
    src3, cand = torch.tensor([busiest, 1, 2], device=DEV), torch.arange(N, device=DEV)
    for g, w in zip(T.pairset_select(ps.table, src3, cand, N), ps.select(src3, cand)):
        assert torch.equal(g, w)
    ns, nd = torch.tensor([1, 2, 49], device=DEV), torch.tensor([busiest, 2, 49], device=DEV)
    nt = torch.tensor([9.0, 9.0, 9.0], device=DEV)
    T.pairset_insert(ps.table, ps.status, ns, nd, nt, N)
    ref.insert(ns.cpu().numpy(), nd.cpu().numpy(), nt.cpu().numpy())
    R.assert_state_equal(ps.state(), ref)
    with pytest.raises(RuntimeError, match="capacity / 8"):
        T.pairset_insert(ps.table, ps.status, gs, gd, torch.zeros(gs.numel(), device=DEV), N)


def test_refusals():
    from tgnx import _lib
    from tgnx.pairset import PairSet
    with pytest.raises(ValueError, match="power of two"):
        PairSet(N, 100, device=DEV)
    with pytest.raises(ValueError, match="num_nodes"):
        PairSet((1 << 31) + 1, 64, device=DEV)
    ps = _set()
    with pytest.raises(RuntimeError, match="num_nodes"):           # the C ABI refuses a node space that reaches EMPTY
        _lib.call("tgnx_pairset_insert", ps.table.data_ptr(), 64, 0, 0, 0, 1, 1 << 32, ps.status.data_ptr(),
                  _lib.stream(DEV))
    with pytest.raises(ValueError, match="differ in length"):
        ps.insert([1, 2], [1], [0.0, 0.0])
    with pytest.raises(ValueError, match="one cut per query"):
        ps.lookup([1, 2], [1, 2], since=np.zeros(3, np.float32))
