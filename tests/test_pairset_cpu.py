"""CPU tests of the live pair set's host side (tgnx/pairset.py): the dict reference's own checks, the
growth rule's helpers over simulated schedules, the two documented formulas and the argument checks.  No device."""
import inspect

import numpy as np
import pytest

import pairset_ref as R
from tgnx import pairset as P


# ---------------------------------------------------------------- the reference checks itself
def test_reference_counts_and_stamps():
    ref = R.RefPairSet(5)
    ref.insert([0, 0, 1, 4, 0], [1, 1, 1, 4, 1], [3.0, -1.0, 0.0, 1.6e9, 2.0])
    seen, cnt, tf, tl = ref.lookup([0, 1, 4, 2, 1], [1, 1, 4, 2, 0])
    assert seen.tolist() == [True, True, True, False, False]
    assert cnt.tolist() == [3, 1, 1, 0, 0]
    assert tf[:3].tolist() == [-1.0, 0.0, np.float32(1.6e9)] and tl[:3].tolist() == [3.0, 0.0, np.float32(1.6e9)]
    assert np.isposinf(tf[3]) and np.isneginf(tl[3])
    assert ref.contains([0, 0], [1, 1], since=[3.0, 3.5]).tolist() == [True, False]
    assert ref.n_keys == 3 and ref.t_hi == np.float32(1.6e9)


def test_reference_refuses_nan_and_ids_out_of_range():
    ref = R.RefPairSet(3)
    ref.insert([0, 3, -1, 1], [1, 0, 0, 2], [1.0, 1.0, 1.0, np.nan])
    assert ref.n_keys == 1 and ref.n_invalid == 3 and not ref.contains([1], [2])[0]


def test_reference_select_keeps_candidate_order_and_duplicates():
    ref = R.RefPairSet(6)
    ref.insert([0, 0, 2], [5, 1, 3], [1.0, 2.0, 3.0])
    ptr, ids = ref.select([0, 1, 2], [5, 3, 1, 5, 4])
    assert ptr.tolist() == [0, 3, 3, 4] and ids.tolist() == [5, 1, 5, 3]
    ptr, ids = ref.select([0, 2], [5, 3, 1], since=2.0)
    assert ptr.tolist() == [0, 1, 2] and ids.tolist() == [1, 3]
    assert ref.select([], [1, 2])[0].tolist() == [0] and ref.select([0], [])[0].tolist() == [0, 0]


def test_reference_erase_and_sorted_state():
    ref = R.RefPairSet(4)
    ref.insert([0, 1, 2, 3], [1, 2, 3, 3], [1.0, 2.0, 3.0, 4.0])
    assert ref.erase([3]) == 2
    keys, cnt, tf, tl = ref.sorted_state()
    assert keys.tolist() == [(0 << 32) | 1, (1 << 32) | 2] and cnt.tolist() == [1, 1]


def test_reference_edgebank_rules_and_repeat_mask():
    src, dst = np.array([0, 0, 0, 1, 0, 1]), np.array([1, 1, 2, 2, 1, 2])
    t = np.array([0.0, 1.0, 2.0, 3.0, 10.0, 11.0], np.float32)
    assert R.repeat_mask(src, dst, t, 0, 6, 2).tolist() == [False, False, False, False, True, True]
    assert R.repeat_mask(src, dst, t, 0, 6, 6).tolist() == [False] * 6
    negs = np.array([[2], [1]])
    # rows 4, 5 against the bank of rows [0, 4): both positives held; row 4's negative (0, 2) too, row 5's (1, 1) not
    assert R.edgebank_stream_ref(src, dst, t, 4, 6, 2, negs) == pytest.approx((1 / 1.5 + 1.0) / 2)
    # a window of 1.5 before t_hi = 3 keeps (0, 2) and (1, 2) only: row 4's positive is out, its negative in
    assert R.edgebank_stream_ref(src, dst, t, 4, 6, 2, negs, window=1.5) == pytest.approx((1 / 2 + 1.0) / 2)
    assert R.tie_ranks([1.0, 0.0], [[1.0, 0.0], [0.0, 0.0]]).tolist() == [1.5, 2.0]


# ---------------------------------------------------------------- the documented formulas
def test_home_slot_restatements_agree():
    rng = np.random.default_rng(0)
    keys = R.pair_key(rng.integers(0, 1 << 31, 500), rng.integers(0, 1 << 31, 500))
    for cap in (64, 128, 1 << 20):
        got = R.home_slot(keys, cap)
        assert got.min() >= 0 and got.max() < cap
        assert got.tolist() == [P.home_slot(int(k), cap) for k in keys]
    s, d = R.colliding_keys(64, 63, 32, 50)
    assert len(set(zip(s.tolist(), d.tolist()))) == 32 and (R.home_slot(R.pair_key(s, d), 64) == 63).all()


def test_ordered_u32_is_monotone():
    t = np.array([-1.0, -0.0, 0.0, 1e-30, 1.0, 1.6e9], np.float32)
    u = R.ordered_u32(t).astype(np.int64)
    assert (np.diff(u) >= 0).all()
    assert (np.diff(u) > 0).tolist() == (np.diff(t) > 0).tolist()          # strict exactly where the floats differ
    assert u[1] == u[2] and 0 < u.min() and u.max() < 0xFFFFFFFF              # -0.0 is 0.0; the identities stay free
    rng = np.random.default_rng(1)
    x = np.sort(rng.standard_normal(1000).astype(np.float32) * np.float32(1e6))
    assert (np.diff(R.ordered_u32(x).astype(np.int64)) >= 0).all()


# ---------------------------------------------------------------- the growth rule
def _simulate(events, distinct, chunk=None, cap=64):
    """Drive needs_read / grown_capacity as PairSet._make_room does.  distinct: every event is a new pair, else every
    event is the same pair.  Returns (events inserted at each read, capacities at each read, final capacity)."""
    ub = n_keys = inserted = 0
    reads, caps = [], []
    while inserted < events:
        n = min(P.max_chunk(cap) if chunk is None else min(chunk, P.max_chunk(cap)), events - inserted)
        if P.needs_read(ub, n, cap):
            reads.append(inserted)
            cap = P.grown_capacity(n_keys, cap)
            caps.append(cap)
            ub = n_keys
        assert ub + n <= cap // 2                            # the load stays at or below 1/2 whatever the batch holds
        ub += n
        inserted += n
        n_keys = inserted if distinct else 1
        assert n_keys <= ub and n_keys <= cap // 2
    return reads, caps, cap


@pytest.mark.parametrize("distinct", [True, False])
@pytest.mark.parametrize("chunk", [None, 1, 7, 200])
def test_growth_schedule_load_and_read_spacing(distinct, chunk):
    cap0 = P.min_capacity(chunk or 8)
    reads, caps, cap = _simulate(100_000, distinct, chunk, cap0)
    assert reads, "a 100,000-event schedule must read at least once"
    prev, prev_cap = 0, cap0
    for at, c in zip(reads, caps):
        assert at - prev >= prev_cap // 8, (at, prev, prev_cap)   # two reads are >= capacity / 8 events apart
        prev, prev_cap = at, c
    if distinct:
        assert cap >= 2 * 100_000 and len(set(caps)) > 3     # it grew, and never past what load 1/4 asks for twice
        assert cap <= 8 * P.next_pow2(100_000)
    else:
        assert cap == cap0                                   # one pair never grows the table


def test_helpers():
    assert [P.next_pow2(n) for n in (0, 1, 2, 3, 64, 65)] == [1, 1, 2, 4, 64, 128]
    assert P.min_capacity(1) == 64 and P.min_capacity(200) == 2048 and P.min_capacity(2048) == 16384
    assert P.max_chunk(64) == 8 and P.max_chunk(P.min_capacity(200)) >= 200
    assert P.grown_capacity(16, 64) == 64 and P.grown_capacity(17, 64) == 128 and P.grown_capacity(1000, 64) == 4096
    assert not P.needs_read(24, 8, 64) and P.needs_read(25, 8, 64)


# ---------------------------------------------------------------- argument checks
def test_argument_checks():
    for bad in (0, 32, 63, 96, -64):
        with pytest.raises(ValueError, match="power of two"):
            P.check_capacity(bad)
    assert P.check_capacity(64) == 64
    for bad in (0, -1, (1 << 31) + 1, 1 << 32):
        with pytest.raises(ValueError, match="num_nodes"):
            P.check_num_nodes(bad)
    assert P.check_num_nodes(1 << 31) == 1 << 31
    with pytest.raises(ValueError, match="missing"):
        P.check_state({"format": 1})


def test_signatures():
    from tgnx import tgn_epoch
    from tgnx.tgn import TgnEngine
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(P.PairSet.__init__) == ["self", "num_nodes", "capacity", "device"]
    assert par(P.PairSet.select) == ["self", "src", "candidates", "since"]
    assert par(P.PairSet.lookup) == ["self", "src", "dst", "since"]
    for f in (TgnEngine.recommend_filtered, TgnEngine.rank, TgnEngine.rank_events):
        sig = inspect.signature(f).parameters
        for k in ("exclude_history", "history_since"):
            assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default in (False, None)
    for name in ("enable_pair_history", "disable_pair_history", "record_pairs", "clear_pair_history", "seen",
                 "pair_stats", "pair_history_state", "load_pair_history_state", "history_exclusions"):
        assert callable(getattr(TgnEngine, name))
    sig = inspect.signature(tgn_epoch.rank_stream).parameters
    assert sig["split_history"].default is False and sig["exclude_history"].default is False
    assert par(tgn_epoch.edgebank_stream)[:6] == ["loader", "lo", "hi", "batch", "negs", "window"]
    assert tgn_epoch.edgebank_window(np.array([10.0, 110.0])) == pytest.approx(15.0)
    import pyg_epoch_utils
    for name in ("edgebank_stream", "edgebank_window", "enable_pair_history", "seen"):
        assert getattr(pyg_epoch_utils, name) is getattr(tgn_epoch, name)
