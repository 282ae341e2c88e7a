"""numpy restatement of the device pair index and the hist_rnd evaluation-negative generator (test infrastructure
only), written from the contract in DESIGN §3b-12; it calls nothing of the library.  The counter-based draws use
tests/dropout_ref.hash4 (csrc/tgnx_common.h restated).

  pair_index(src, dst, N)            -> indptr int64[N+1], indices int64[nnz], first int64[nnz]
  contains(index, src, dst, before)  -> bool[n]: the pair occurred at a row < before
  hist_rnd(...)                      -> rows int64[n, k], k_hist int32[n], status int64[4], info (per-row path record)

Per event row e (source s), sequentially:
  P  = destinations of rows j in [lo, hi) with src[j] == s and t[j] == t[e]
  Hc = s's index row restricted to first < hist_hi (ascending);  Hn = Hc \\ P;  X = Hc | P;  valid = pool \\ X
  historical: all of Hn when |Hn| <= q, else draws a = 0, 1, ...: v = Hc[((hash4(seed, TAG_HIST, e, a) >> 11) * |Hc|) >> 53],
              accepted when v not in P and new, until q are accepted
  random:     k_r = k - k_h; |valid| >= k_r: draws v = pool[((hash4(seed, TAG_RND, e, a) >> 11) * |pool|) >> 53], accepted
              when v not in X and new, until k_r; 0 < |valid| < k_r: valid[i mod |valid|]; |valid| == 0: unusable (-1)
  a draw loop stops after max_draws draws (0: 16 * target + 256) and fills up with the smallest ids not yet taken
  each part is stored ascending; status = [first unusable output row or -1, rows with a historical fill-up, rows with
  a random fill-up, rows filled cyclically]
"""
from __future__ import annotations

import numpy as np

from dropout_ref import hash4

TAG_HIST = 0x68697374   # "hist"
TAG_RND = 0x726E6473    # "rnds"
MAX_K = 1024


def pair_index(src, dst, num_nodes: int):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    key = (src.astype(np.uint64) << np.uint64(32)) | dst.astype(np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    first = np.full(uk.shape[0], np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, inv, np.arange(src.shape[0], dtype=np.int64))
    s = (uk >> np.uint64(32)).astype(np.int64)
    indptr = np.zeros(num_nodes + 1, np.int64)
    np.add.at(indptr, s + 1, 1)
    return np.cumsum(indptr), (uk & np.uint64(0xFFFFFFFF)).astype(np.int64), first


def contains(index, src, dst, before=None):
    indptr, indices, first = index
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    cut = np.broadcast_to(np.iinfo(np.int64).max if before is None else np.asarray(before, np.int64), src.shape)
    out = np.zeros(src.shape[0], bool)
    for i, (s, d) in enumerate(zip(src, dst)):
        if 0 <= s < indptr.shape[0] - 1:
            a, b = indptr[s], indptr[s + 1]
            p = a + np.searchsorted(indices[a:b], d)
            out[i] = p < b and indices[p] == d and first[p] < cut[i]
    return out


def draw_index(seed: int, tag: int, e: int, a, n: int):
    """((hash4(seed, tag, e, a) >> 11) * n) >> 53 with the full 117-bit product (a may be an array)."""
    h = np.atleast_1d(hash4(seed, tag, e, a)) >> np.uint64(11)
    return np.array([(int(x) * int(n)) >> 53 for x in h], np.int64)


def _draw_part(seed, tag, e, table, banned, target, max_draws):
    """The first `target` distinct values of the draw sequence over `table` that are not in `banned`, at most
    max_draws draws; returns (accepted list, draws made)."""
    cap = max_draws if max_draws > 0 else 16 * target + 256
    got, seen, a = [], set(), 0
    while len(got) < target and a < cap:
        n = min(256, cap - a)
        for j, i in enumerate(draw_index(seed, tag, e, np.arange(a, a + n, dtype=np.uint64), len(table))):
            v = int(table[i])
            if v not in banned and v not in seen:
                seen.add(v)
                got.append(v)
                if len(got) == target:
                    return got, a + j + 1
        a += n
    return got, a


def hist_rnd(src, dst, t, lo, hi, k, q, hist_hi, pool, seed, max_draws=0, index=None, rows=None):
    src, dst, t = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(t)
    pool = np.asarray(pool, np.int64)
    if not (0 < k <= MAX_K and 0 <= q <= k):
        raise ValueError("k must be in [1, 1024] and q in [0, k]")
    if index is None:
        index = pair_index(src, dst, int(max(src.max(), dst.max())) + 1)
    indptr, indices, first = index
    r0, r1 = (lo, hi) if rows is None else rows
    n = r1 - r0
    out = np.full((n, k), -1, np.int64)
    k_hist = np.zeros(n, np.int32)
    status = np.array([-1, 0, 0, 0], np.int64)
    info = dict(take_all=np.zeros(n, bool), n_hc=np.zeros(n, np.int64), n_p=np.zeros(n, np.int64),
                hist_draws=np.zeros(n, np.int64), rnd_draws=np.zeros(n, np.int64), cyclic=np.zeros(n, bool),
                empty=np.zeros(n, bool), n_valid=np.zeros(n, np.int64))
    ssrc, st, sdst = src[lo:hi], t[lo:hi], dst[lo:hi]
    for r, e in enumerate(range(r0, r1)):
        s = int(src[e])
        P = set(sdst[(ssrc == s) & (st == t[e])].tolist())
        a, b = (indptr[s], indptr[s + 1]) if 0 <= s < indptr.shape[0] - 1 else (0, 0)
        Hc = indices[a:b][first[a:b] < hist_hi]
        Hn = [int(v) for v in Hc if int(v) not in P]
        X = set(Hc.tolist()) | P
        valid = pool[~np.isin(pool, np.fromiter(X, np.int64, len(X)))]
        info["n_hc"][r], info["n_p"][r], info["n_valid"][r] = len(Hc), len(P), len(valid)
        if len(Hn) <= q:
            hist = Hn
            info["take_all"][r] = True
        else:
            hist, info["hist_draws"][r] = _draw_part(seed, TAG_HIST, e, Hc, P, q, max_draws)
            if len(hist) < q:
                status[1] += 1
                hist = hist + [v for v in Hn if v not in set(hist)][:q - len(hist)]
        kh = len(hist)
        k_hist[r] = kh
        out[r, :kh] = sorted(hist)
        kr = k - kh
        if kr == 0:
            continue
        if len(valid) == 0:
            info["empty"][r] = True
            if status[0] < 0:
                status[0] = r
        elif len(valid) < kr:
            info["cyclic"][r] = True
            status[3] += 1
            out[r, kh:] = np.sort(valid[np.arange(kr) % len(valid)])
        else:
            rnd, info["rnd_draws"][r] = _draw_part(seed, TAG_RND, e, pool, X, kr, max_draws)
            if len(rnd) < kr:
                status[2] += 1
                rnd = rnd + [int(v) for v in valid if int(v) not in set(rnd)][:kr - len(rnd)]
            out[r, kh:] = sorted(rnd)
    return out, k_hist, status, info


def stream(n_src, n_dst, E, tmax, zs, zd, seed=3):
    """The test streams' recipe: Zipf-ranked sources and destinations, sorted integer timestamps (drawn in that order)."""
    rng = np.random.default_rng(seed)
    ps = np.arange(1, n_src + 1, dtype=np.float64) ** -zs
    pd = np.arange(1, n_dst + 1, dtype=np.float64) ** -zd
    src = rng.choice(n_src, E, p=ps / ps.sum()).astype(np.int64)
    dst = (n_src + rng.choice(n_dst, E, p=pd / pd.sum())).astype(np.int64)
    t = np.sort(rng.integers(0, tmax + 1, E)).astype(np.float64)
    return src, dst, t


# name -> (n_src, n_dst, E, k, q, tmax, zs, zd, rows)
SHAPES = {"A": (48, 80, 600, 20, 10, 150, 1.0, 0.6, 96),
          "B2": (48, 36, 600, 20, 10, 150, 1.0, 0.6, 96),
          "B": (48, 16, 600, 20, 10, 150, 1.0, 0.6, 96),
          "C": (4, 3000, 6000, 999, 499, 2000, 0.5, 0.0, 24),
          "D": (24, 60, 400, 16, 8, 0, 1.0, 0.6, 96)}
SEED = 7
_cache = {}


def case(name, max_draws=0):
    """(stream arrays and call arguments, the restatement's result) of a named shape, computed once and shared; the
    arrays are read-only."""
    key = (name, max_draws)
    if key not in _cache:
        n_src, n_dst, E, k, q, tmax, zs, zd, rows = SHAPES[name]
        src, dst, t = stream(n_src, n_dst, E, tmax, zs, zd)
        lo = int(0.7 * E)
        args = dict(src=src, dst=dst, t=t, lo=lo, hi=lo + rows, k=k, q=q, hist_hi=lo, pool=np.unique(dst), seed=SEED,
                    num_nodes=n_src + n_dst)
        res = hist_rnd(src, dst, t, lo, lo + rows, k, q, lo, args["pool"], SEED, max_draws=max_draws)
        for x in (src, dst, t, args["pool"]) + res[:3]:
            x.setflags(write=False)
        _cache[key] = (args, res)
    return _cache[key]
