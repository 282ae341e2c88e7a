"""A dict-based restatement of the live pair set (include/tgnx.h tgnx_pairset_*), for the tests.

RefPairSet maps (src, dst) -> [count, t_first, t_last] with float32 stamps compared in numpy's order; a NaN stamp or an
id outside [0, num_nodes) is refused (counted, never inserted).  select / erase, the EdgeBank rules and the novel /
repeat mask are restated over it.  home_slot / ordered_u32 restate the header's two formulas in numpy."""
import numpy as np

HASH_MULT = np.uint64(0x9E3779B97F4A7C15)


def home_slot(key, capacity):
    """(key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2(capacity)) for uint64 keys (array or scalar)."""
    log2cap = int(capacity).bit_length() - 1
    assert 1 << log2cap == int(capacity)
    with np.errstate(over="ignore"):
        return ((np.asarray(key, dtype=np.uint64) * HASH_MULT) >> np.uint64(64 - log2cap)).astype(np.int64)


def pair_key(src, dst):
    return (np.asarray(src, dtype=np.uint64) << np.uint64(32)) | np.asarray(dst, dtype=np.uint64)


def ordered_u32(t):
    """The order-preserving uint32 of float32 stamps: -0.0 taken as 0.0, then ~bits when the sign bit is set, else
    bits | 0x80000000."""
    t = np.asarray(t, dtype=np.float32) + np.float32(0.0)          # (-0.0 + 0.0 = +0.0)
    b = t.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def colliding_keys(capacity, slot, n, num_nodes, skip=()):
    """The first n keys (src << 32 | dst, ids below num_nodes, in (src, dst) order) whose home slot is `slot`, as
    (src, dst) int64 arrays; pairs in `skip` (a set of tuples) are passed over."""
    s, d = np.divmod(np.arange(num_nodes * num_nodes, dtype=np.int64), num_nodes)
    hit = home_slot(pair_key(s, d), capacity) == slot
    s, d = s[hit], d[hit]
    keep = [i for i in range(s.size) if (int(s[i]), int(d[i])) not in skip][:n]
    assert len(keep) == n, f"only {len(keep)} keys of home slot {slot} among {num_nodes}^2 pairs"
    return s[keep], d[keep]


class RefPairSet:
    def __init__(self, num_nodes):
        self.num_nodes = int(num_nodes)
        self.map = {}
        self.n_invalid = 0
        self.t_hi = None                                # the largest stamp inserted so far

    def insert(self, src, dst, t):
        t = np.asarray(t, dtype=np.float32)
        for s, d, ti in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), t):
            if not (0 <= s < self.num_nodes and 0 <= d < self.num_nodes) or np.isnan(ti):
                self.n_invalid += 1
                continue
            e = self.map.get((s, d))
            if e is None:
                self.map[(s, d)] = [1, ti, ti]
            else:
                e[0] += 1
                e[1] = min(e[1], ti)
                e[2] = max(e[2], ti)
            self.t_hi = ti if self.t_hi is None else max(self.t_hi, ti)

    @property
    def n_keys(self):
        return len(self.map)

    def lookup(self, src, dst, since=None):
        """(seen bool[n], count int64[n], t_first float32[n], t_last float32[n]); 0 / +inf / -inf when absent."""
        src, dst = np.asarray(src).tolist(), np.asarray(dst).tolist()
        n = len(src)
        cut = np.full(n, -np.inf, np.float32) if since is None else np.broadcast_to(np.asarray(since, np.float32), (n,))
        seen, cnt = np.zeros(n, bool), np.zeros(n, np.int64)
        tf, tl = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
        for i, (s, d) in enumerate(zip(src, dst)):
            e = self.map.get((s, d))
            if e is not None:
                cnt[i], tf[i], tl[i] = e
                seen[i] = bool(e[2] >= cut[i])
        return seen, cnt, tf, tl

    def contains(self, src, dst, since=None):
        return self.lookup(src, dst, since)[0]

    def select(self, src, cand, since=None):
        """(ptr int64[Q + 1], ids): per source the candidates it has met, in candidate order, duplicates kept."""
        src, cand = np.asarray(src).reshape(-1), np.asarray(cand).reshape(-1)
        Q = src.size
        cut = [None] * Q if since is None else np.broadcast_to(np.asarray(since, np.float32), (Q,))
        ptr, ids = np.zeros(Q + 1, np.int64), []
        for q in range(Q):
            hit = self.contains(np.full(cand.size, src[q]), cand, cut[q]) if cand.size else np.zeros(0, bool)
            ids.append(cand[hit])
            ptr[q + 1] = ptr[q] + int(hit.sum())
        return ptr, (np.concatenate(ids) if ids else np.zeros(0, np.int64)).astype(np.int64)

    def erase(self, ids):
        """Drop every pair that names a node of ids; returns how many."""
        ids = set(np.asarray(ids).reshape(-1).tolist())
        gone = [k for k in self.map if k[0] in ids or k[1] in ids]
        for k in gone:
            del self.map[k]
        return len(gone)

    def sorted_state(self):
        """(keys int64 ascending, count int64, t_first float32, t_last float32): the form sets are compared in."""
        items = sorted(self.map.items())
        keys = np.array([(s << 32) | d for (s, d), _ in items], dtype=np.int64)
        cnt = np.array([v[0] for _, v in items], dtype=np.int64)
        tf = np.array([v[1] for _, v in items], dtype=np.float32)
        tl = np.array([v[2] for _, v in items], dtype=np.float32)
        return keys, cnt, tf, tl


def assert_state_equal(state, ref):
    """A PairSet.state() dict against a RefPairSet, exactly."""
    keys, cnt, tf, tl = ref.sorted_state()
    assert np.array_equal(state["keys"].cpu().numpy(), keys)
    assert np.array_equal(state["count"].cpu().numpy(), cnt)
    assert np.array_equal(state["t_first"].cpu().numpy(), tf)
    assert np.array_equal(state["t_last"].cpu().numpy(), tl)


def tie_ranks(pos, neg):
    """1 + #(neg > pos) + #(neg == pos) / 2 per row: the tie-averaged rank tgnx.data.Evaluator uses."""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64)
    return 0.5 * ((neg > pos[:, None]).sum(1) + (neg >= pos[:, None]).sum(1)) + 1.0


def edgebank_stream_ref(src, dst, t, lo, hi, batch, negs, window=None):
    """Prequential EdgeBank: the bank holds rows [0, lo); every batch is scored against the bank before it (score 1
    iff the pair is held and, with a window, t_last >= float32(t_hi - window), t_hi the largest stamp inserted so far),
    then inserted.  The mean over batches of the batch MRR."""
    src, dst, t = np.asarray(src), np.asarray(dst), np.asarray(t, np.float32)
    num_nodes = int(max(src.max(), dst.max(), np.asarray(negs).max())) + 1
    bank = RefPairSet(num_nodes)
    bank.insert(src[:lo], dst[:lo], t[:lo])
    K = negs.shape[1]
    out = []
    for a in range(lo, hi, batch):
        b = min(batch, hi - a)
        if window is None:
            since = None
        elif bank.t_hi is None:
            since = np.float32(np.inf)
        else:
            since = np.float32(bank.t_hi - np.float32(window))
        s = src[a:a + b]
        pos = bank.contains(s, dst[a:a + b], since).astype(np.float64)
        neg = bank.contains(np.repeat(s, K), negs[a - lo:a - lo + b].reshape(-1), since).reshape(b, K).astype(np.float64)
        out.append(float((1.0 / tie_ranks(pos, neg)).mean()))
        bank.insert(s, dst[a:a + b], t[a:a + b])
    return float(np.mean(out))


def repeat_mask(src, dst, t, lo, hi, batch, upto=0):
    """bool[hi - lo]: the event's pair was in the bank before its batch.  The bank starts from rows [upto, lo) (what
    the engine observed, and so recorded, before the ranked range)."""
    src, dst, t = np.asarray(src), np.asarray(dst), np.asarray(t, np.float32)
    bank = RefPairSet(int(max(src.max(), dst.max())) + 1)
    bank.insert(src[upto:lo], dst[upto:lo], t[upto:lo])
    out = np.zeros(hi - lo, bool)
    for a in range(lo, hi, batch):
        b = min(batch, hi - a)
        out[a - lo:a - lo + b] = bank.contains(src[a:a + b], dst[a:a + b])
        bank.insert(src[a:a + b], dst[a:a + b], t[a:a + b])
    return out
