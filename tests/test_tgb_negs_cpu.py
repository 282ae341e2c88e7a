"""CPU checks of the numpy restatement of the hist_rnd evaluation negatives (tests/tgb_negs_ref.py), which the GPU
tests compare the device against bit for bit: the contract's set and count properties on every test stream, a
hand-computed first draw, uniformity of the random part over `valid`, and the path counts of each stream — so the
GPU tests are known to cover every path of the kernel, and the fill-up only where it is forced."""
import numpy as np
import pytest

import tgb_negs_ref as R
from dropout_ref import hash4, mix64

NAMES = list(R.SHAPES)


def _sets(a, e):
    """(P, Hc, Hn, X, valid) of event row e, by brute force on the raw arrays."""
    src, dst, t, lo, hi = a["src"], a["dst"], a["t"], a["lo"], a["hi"]
    s = src[e]
    P = {int(dst[j]) for j in range(lo, hi) if src[j] == s and t[j] == t[e]}
    Hc = sorted({int(dst[j]) for j in range(a["hist_hi"]) if src[j] == s})
    Hn = [v for v in Hc if v not in P]
    X = set(Hc) | P
    valid = [int(v) for v in a["pool"] if int(v) not in X]
    return P, Hc, Hn, X, valid


@pytest.mark.parametrize("name", NAMES)
def test_rows_obey_the_contract(name):
    a, (rows, k_hist, status, info) = R.case(name)
    k, q = a["k"], a["q"]
    assert rows.shape == (a["hi"] - a["lo"], k) and k_hist.shape == (rows.shape[0],)
    for r, e in enumerate(range(a["lo"], a["hi"])):
        P, Hc, Hn, X, valid = _sets(a, e)
        kh = int(k_hist[r])
        assert kh == min(q, len(Hn)), (r, kh)
        hist, rnd = rows[r, :kh].tolist(), rows[r, kh:].tolist()
        assert set(hist) <= set(Hn) and hist == sorted(hist) and len(set(hist)) == kh, r
        assert info["n_valid"][r] == len(valid) and info["n_hc"][r] == len(Hc) and info["n_p"][r] == len(P), r
        if info["empty"][r]:
            assert not valid and rnd == [-1] * (k - kh), r
            continue
        assert len(rnd) == k - kh and all(v >= 0 for v in rows[r]), r          # every row has k entries
        assert not set(rnd) & X and set(rnd) <= set(valid) and rnd == sorted(rnd), r
        if info["cyclic"][r]:
            assert len(valid) < k - kh and set(rnd) == set(valid), r
            cnt = np.bincount(np.searchsorted(valid, rnd), minlength=len(valid))
            want = (k - kh) // len(valid) + (np.arange(len(valid)) < (k - kh) % len(valid))
            assert np.array_equal(cnt, want), r                                  # valid[i mod |valid|]
        else:
            assert len(set(rnd)) == k - kh, r
    first_empty = np.flatnonzero(info["empty"])
    assert status[0] == (first_empty[0] if first_empty.size else -1)
    assert status[3] == info["cyclic"].sum()


# the path counts each stream was chosen for (observed on the restatement, asserted so that a change of recipe that
# loses a path fails here): take-all / drawn rows, sources without history, rows with several same-time positives,
# cyclic rows, empty rows, longest historical / random draw loop
PATHS = {"A": (33, 63, 1, 26, 0, 0, 25, 48), "B2": (36, 60, 1, 26, 26, 0, 30, 76), "B": (59, 37, 1, 26, 70, 26, 27, 0),
         "C": (0, 24, 0, 10, 0, 0, 927, 1191), "D": (24, 72, 0, 93, 0, 0, 32, 84)}


@pytest.mark.parametrize("name", NAMES)
def test_path_counts(name):
    a, (rows, k_hist, status, info) = R.case(name)
    sl = slice(a["lo"], a["hi"])
    same = [int(((a["src"][sl] == a["src"][e]) & (a["t"][sl] == a["t"][e])).sum()) for e in range(a["lo"], a["hi"])]
    got = (int(info["take_all"].sum()), int((~info["take_all"]).sum()), int((info["n_hc"] == 0).sum()),
           int(sum(c > 1 for c in same)), int(info["cyclic"].sum()), int(info["empty"].sum()),
           int(info["hist_draws"].max()), int(info["rnd_draws"].max()))
    assert got == PATHS[name], got
    assert status[1] == 0 and status[2] == 0                  # no fill-up at the default draw cap
    if name == "C":                                           # many 256-draw chunks against a full accepted set
        assert info["hist_draws"].max() > 3 * 256 and info["rnd_draws"].max() > 4 * 256


def test_forced_fill_up():
    """max_draws = 8 on shape A: every drawn historical part and every random part stops short and is filled up with
    the smallest ids not yet taken; the contract's properties still hold."""
    a, (rows, k_hist, status, info) = R.case("A", 8)
    assert status[1] == 63 and status[2] == 96 and status[0] == -1 and status[3] == 0
    a0, (rows0, k_hist0, _, _) = R.case("A")
    assert np.array_equal(k_hist, k_hist0) and not np.array_equal(rows, rows0)
    for r, e in enumerate(range(a["lo"], a["hi"])):
        P, Hc, Hn, X, valid = _sets(a, e)
        kh = int(k_hist[r])
        hist, rnd = rows[r, :kh].tolist(), rows[r, kh:].tolist()
        assert set(hist) <= set(Hn) and len(set(hist)) == kh and len(set(rnd)) == a["k"] - kh and not set(rnd) & X
        # at most 8 draws: at least target - 8 of the picks are the smallest ids left
        if a["k"] - kh > 8:
            assert len(set(rnd) & set(valid[:a["k"] - kh])) >= a["k"] - kh - 8, r


def test_halves_and_time_shift_give_the_same_rows():
    """No (source, timestamp) group of shape A straddles the middle of the split, so two half-range calls (history
    still cut at lo) see the same P for every row; shifting t by 1.6e9 keeps every float64 stamp distinct (float32
    would merge them: spacing 128 at that magnitude)."""
    a, (rows, k_hist, status, _) = R.case("A")
    lo, hi = a["lo"], a["hi"]
    mid = (lo + hi) // 2
    s, t = a["src"], a["t"]
    assert not [(i, j) for i in range(lo, mid) for j in range(mid, hi) if s[i] == s[j] and t[i] == t[j]]
    args = (a["k"], a["q"], a["hist_hi"], a["pool"], a["seed"])
    h0 = R.hist_rnd(a["src"], a["dst"], t, lo, mid, *args)
    h1 = R.hist_rnd(a["src"], a["dst"], t, mid, hi, *args)
    assert np.array_equal(np.concatenate([h0[0], h1[0]]), rows) and np.array_equal(np.concatenate([h0[1], h1[1]]), k_hist)
    shifted = R.hist_rnd(a["src"], a["dst"], 1.6e9 + t, lo, hi, *args)
    assert np.array_equal(shifted[0], rows)
    t32 = (1.6e9 + t).astype(np.float32)
    assert np.unique(t32[lo:hi]).size < np.unique(t[lo:hi]).size


def test_tags_and_first_draw_by_hand():
    """The first historical and random draw of one drawn row, computed here from splitmix64 written out, against the
    restatement's draw_index and against what the row accepted."""
    assert R.TAG_HIST == int.from_bytes(b"hist", "big") and R.TAG_RND == int.from_bytes(b"rnds", "big")
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    assert int(mix64(12345)) == mix(12345)
    a, (rows, k_hist, status, info) = R.case("A")
    r = int(np.flatnonzero(~info["take_all"])[0])
    e = a["lo"] + r
    P, Hc, Hn, X, valid = _sets(a, e)
    for tag, table, banned, part in ((R.TAG_HIST, Hc, P, rows[r, :k_hist[r]]), (R.TAG_RND, a["pool"], X, rows[r, k_hist[r]:])):
        h = mix(R.SEED ^ mix(tag ^ mix(e ^ mix(0))))
        assert int(hash4(R.SEED, tag, e, 0)) == h
        idx = ((h >> 11) * len(table)) >> 53
        assert 0 <= idx < len(table) and int(R.draw_index(R.SEED, tag, e, 0, len(table))[0]) == idx
        v = int(table[idx])
        assert (v in part) == (v not in banned)             # draw 0 is accepted iff it is not banned


def test_random_part_is_uniform_over_valid():
    """χ² of shape A's accepted random values pooled by their rank in the row's `valid`: every row of the split at the
    fixed generator seeds 100..139.  A row accepts k_r of its |valid| values without replacement, so under uniform
    draws each rank is hit with probability p = k_r / |valid| per row and seed (variance p (1 - p)); the statistic
    Σ_rank (obs - Σ p)² / Σ p (1 - p) over the ranks every row has (each term has expectation 1; the ranks of a row
    are negatively correlated, which only narrows the sum) is compared with the 0.999 quantile of χ² with that many
    degrees of freedom (Wilson-Hilferty)."""
    a, (_, k_hist, _, info) = R.case("A")
    lo, hi = a["lo"], a["hi"]
    n_common = int(info["n_valid"].min())
    obs = np.zeros(n_common)
    exp = np.zeros(n_common)
    var = np.zeros(n_common)
    idx = R.pair_index(a["src"], a["dst"], a["num_nodes"])
    valid_of = [np.array(_sets(a, e)[4]) for e in range(lo, hi)]
    for seed in range(100, 140):
        rows, kh, _, _ = R.hist_rnd(a["src"], a["dst"], a["t"], lo, hi, a["k"], a["q"], a["hist_hi"], a["pool"], seed,
                                    index=idx)
        for r in range(hi - lo):
            rk = np.searchsorted(valid_of[r], rows[r, kh[r]:])
            obs += np.bincount(rk[rk < n_common], minlength=n_common)
            p = (a["k"] - kh[r]) / len(valid_of[r])
            exp += p
            var += p * (1 - p)
    chi2 = float(((obs - exp) ** 2 / var).sum())
    df = n_common
    z999 = 3.0902323061678132
    crit = df * (1 - 2 / (9 * df) + z999 * np.sqrt(2 / (9 * df))) ** 3
    print(f"chi2 {chi2:.1f} df {df} crit {crit:.1f}")
    assert chi2 < crit, (chi2, crit)


def test_pair_index_and_contains_restatement():
    a, _ = R.case("A")
    src, dst = a["src"], a["dst"]
    indptr, indices, first = R.pair_index(src, dst, a["num_nodes"])
    assert indptr[-1] == indices.size == len({(int(s), int(d)) for s, d in zip(src, dst)})
    for s in range(a["num_nodes"]):
        row = indices[indptr[s]:indptr[s + 1]]
        assert np.array_equal(row, np.unique(dst[src == s]))
        for d, f in zip(row, first[indptr[s]:indptr[s + 1]]):
            assert f == np.flatnonzero((src == s) & (dst == d))[0]
    cut = 300
    got = R.contains((indptr, indices, first), src[:400], dst[:400], before=cut)
    seen = {(int(s), int(d)) for s, d in zip(src[:cut], dst[:cut])}
    assert np.array_equal(got, [(int(s), int(d)) in seen for s, d in zip(src[:400], dst[:400])])


def test_neg_strategy_env(monkeypatch):
    """TGNX_EVAL_NEG_STRATEGY: unset / uniform keep the uniform tables, hist_rnd without a device says why it cannot
    run, anything else is refused."""
    import torch

    from tgnx import data
    monkeypatch.setenv("TGNX_SYNTH_EVENTS", "600")
    monkeypatch.setenv("TGNX_EVAL_NEGS", "5")
    monkeypatch.delenv("TGNX_EVAL_NEG_STRATEGY", raising=False)
    base = data._load("tgbl-wiki")[6]
    monkeypatch.setenv("TGNX_EVAL_NEG_STRATEGY", "uniform")
    same = data._load("tgbl-wiki")[6]
    assert all(np.array_equal(base[k], same[k]) for k in ("val_neg", "test_neg"))
    monkeypatch.setenv("TGNX_EVAL_NEG_STRATEGY", "hist_rnd")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device is visible"):
        data._load("tgbl-wiki")
    monkeypatch.setenv("TGNX_EVAL_NEG_STRATEGY", "historical")
    with pytest.raises(ValueError, match="TGNX_EVAL_NEG_STRATEGY"):
        data._load("tgbl-wiki")
