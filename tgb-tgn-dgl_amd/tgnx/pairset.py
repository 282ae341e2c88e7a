"""A live (source, destination) pair set on the device (include/tgnx.h tgnx_pairset_*; csrc/tgnx_pairset.hip; DESIGN
§3b-14 has the contract, tests/pairset_ref.py restates it as a dict).

    ps = PairSet(num_nodes)
    ps.insert(src, dst, t)                       # one launch per chunk; may read the host on the growth schedule
    seen, count, t_first, t_last = ps.lookup(src, dst)
    ptr, ids = ps.select(src, candidates)        # per source the candidates it has met: the operators' `exclude`
    ps.erase_nodes(ids); ps.state(); ps.load_state(state); ps.to_pair_history()

An open-addressing hash table keyed by src << 32 | dst that holds, per pair, the occurrence count and the first and
last float32 timestamp.  It names no event rows, so it survives compact_events(); tgnx.tgb_negs.PairHistory is the
static CSR over a whole table it complements.  The contents are a function of the multiset of inserted events (every
update is a commutative integer atomic); the slot layout is not, and nothing returned here depends on it.

Growth rule (pure helpers below, tests/test_pairset_cpu.py): the load never exceeds 1/2.  The host keeps an upper
bound `ub` on n_keys (+= n per insert).  When ub + n > capacity / 2 it reads n_keys once; if n_keys > capacity / 4 the
capacity doubles until that no longer holds (allocate, rehash, swap); then ub = n_keys.  One insert launch takes at
most capacity / 8 events (longer inputs are chunked), so two host reads are at least capacity / 8 inserted events
apart.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

MIN_CAPACITY = 64
MAX_NODES = 1 << 31     # (the C ABI takes ids below 2^32 - 1; the sorted int64 keys of state() want the sign bit clear)
STATE_FORMAT = 1
STATE_KEYS = ("format", "num_nodes", "keys", "count", "t_first", "t_last")
HASH_MULT = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------- pure helpers (no device)
def next_pow2(n: int) -> int:
    n = max(int(n), 1)
    return 1 << (n - 1).bit_length()


def check_capacity(capacity: int) -> int:
    capacity = int(capacity)
    if capacity < MIN_CAPACITY or capacity & (capacity - 1):
        raise ValueError(f"PairSet: capacity = {capacity} must be a power of two >= {MIN_CAPACITY}")
    return capacity


def check_num_nodes(num_nodes: int) -> int:
    num_nodes = int(num_nodes)
    if not 0 < num_nodes <= MAX_NODES:
        raise ValueError(f"PairSet: num_nodes = {num_nodes} outside [1, 2^31] (a key is src << 32 | dst and the all-ones "
                         "word is EMPTY)")
    return num_nodes


def min_capacity(max_batch: int) -> int:
    """The smallest capacity whose insert chunk (capacity / 8) takes a batch of max_batch events in one launch."""
    return max(MIN_CAPACITY, next_pow2(8 * int(max_batch)))


def max_chunk(capacity: int) -> int:
    """Events per insert launch."""
    return int(capacity) // 8


def needs_read(ub: int, n: int, capacity: int) -> bool:
    """Inserting n more events could take the load past 1/2: read n_keys first."""
    return int(ub) + int(n) > int(capacity) // 2


def grown_capacity(n_keys: int, capacity: int) -> int:
    """The capacity after a read: doubled until n_keys <= capacity / 4."""
    capacity = int(capacity)
    while int(n_keys) > capacity // 4:
        capacity *= 2
    return capacity


def home_slot(key: int, capacity: int) -> int:
    """The documented hash: (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2(capacity))."""
    log2cap = int(capacity).bit_length() - 1
    return ((int(key) * HASH_MULT) & 0xFFFFFFFFFFFFFFFF) >> (64 - log2cap)


def check_state(state: dict) -> int:
    """Shape / format checks of a state() dict; returns its row count."""
    missing = [k for k in STATE_KEYS if k not in state]
    if missing:
        raise ValueError(f"PairSet.load_state: missing keys {missing}")
    if int(state["format"]) != STATE_FORMAT:
        raise ValueError(f"PairSet.load_state: format {state['format']} (this build reads {STATE_FORMAT})")
    n = int(state["keys"].numel())
    for k in ("count", "t_first", "t_last"):
        if int(state[k].numel()) != n:
            raise ValueError(f"PairSet.load_state: {k} has {int(state[k].numel())} rows for {n} keys")
    return n


def _p(t):
    return 0 if t is None else t.data_ptr()


class PairSet:
    """The device pair set over node ids [0, num_nodes).  capacity: initial slots (a power of two >= 64); it grows by
    the module's rule.  insert() may read the host (one n_keys read) on that schedule, at most once per capacity / 8
    inserted events; lookup / contains never do; select reads ptr[Q] once to size its output."""

    def __init__(self, num_nodes: int, capacity: int = MIN_CAPACITY, device=None):
        self.num_nodes = check_num_nodes(num_nodes)
        capacity = check_capacity(capacity)
        self.device = _lib.require_device(device)
        self.reads = 0                                   # host reads of n_keys made by the growth rule
        self._alloc(capacity)

    # ------------------------------------------------------------------ storage
    def _new_table(self, capacity: int):
        nb = int(_lib.lib().tgnx_pairset_bytes(capacity))
        if nb == 0:
            raise ValueError(f"PairSet: capacity = {capacity} must be a power of two >= {MIN_CAPACITY}")
        table = torch.empty(nb // 8, dtype=torch.int64, device=self.device)
        _lib.call("tgnx_pairset_init", _p(table), capacity, self._stream())
        return table

    def _alloc(self, capacity: int) -> None:
        self.table = self._new_table(capacity)
        self.capacity = int(capacity)
        self.status = torch.zeros(3, dtype=torch.int64, device=self.device)   # [n_keys, n_invalid, n_overflow]
        self._ub = 0

    def _stream(self):
        return _lib.stream(self.device)

    def _ids(self, x) -> torch.Tensor:
        return torch.as_tensor(x).to(self.device, torch.long).contiguous().view(-1)

    @property
    def n_keys(self) -> int:
        """Distinct pairs held (one host read)."""
        return int(self.status[0])

    def counters(self) -> dict:
        """{"n_keys", "n_invalid", "n_overflow"} (one host read).  n_invalid counts the events insert() skipped."""
        a = self.status.tolist()
        return dict(n_keys=a[0], n_invalid=a[1], n_overflow=a[2])

    def set_num_nodes(self, num_nodes: int) -> None:
        """The id bound follows a node space that grew; ids are stable, nothing moves."""
        num_nodes = check_num_nodes(num_nodes)
        if num_nodes < self.num_nodes:
            raise ValueError(f"PairSet: num_nodes may only grow ({self.num_nodes} -> {num_nodes})")
        self.num_nodes = num_nodes

    def clear(self) -> None:
        """Empty the set in place (the capacity stays)."""
        _lib.call("tgnx_pairset_init", _p(self.table), self.capacity, self._stream())
        self.status.zero_()
        self._ub = 0

    # ------------------------------------------------------------------ growth
    def _rehash(self, capacity: int, drop=None) -> None:
        new = self._new_table(capacity)
        _lib.call("tgnx_pairset_rehash", _p(self.table), self.capacity, _p(new), capacity, _p(drop), self.num_nodes,
                  _p(self.status), self._stream())
        self.table, self.capacity = new, int(capacity)

    def _make_room(self, n: int) -> None:
        """The growth rule ahead of a launch of n <= capacity / 8 events."""
        if needs_read(self._ub, n, self.capacity):
            nk = self.n_keys                                  # (the scheduled host read)
            self.reads += 1
            cap = grown_capacity(nk, self.capacity)
            if cap != self.capacity:
                self._rehash(cap)
            self._ub = nk
        self._ub += n

    def reserve(self, capacity: int) -> None:
        """At least `capacity` slots ahead of time (a rehash when it grows); no host read."""
        capacity = check_capacity(capacity)
        if capacity > self.capacity:
            self._rehash(capacity)

    # ------------------------------------------------------------------ writes
    def insert(self, src, dst, t) -> None:
        """Record the events (src[i], dst[i], t[i]): count += 1, t_first / t_last take the float32 stamp by min / max.
        An id outside [0, num_nodes) or a NaN stamp is skipped and counted (counters()["n_invalid"]).  One launch
        per capacity / 8 events; may read the host on the growth schedule (module docstring)."""
        src, dst = self._ids(src), self._ids(dst)
        t = torch.as_tensor(t).to(self.device, torch.float32).contiguous().view(-1)
        n = int(src.numel())
        if int(dst.numel()) != n or int(t.numel()) != n:
            raise ValueError("PairSet.insert: src, dst and t differ in length")
        self.insert_ptr(src.data_ptr(), dst.data_ptr(), t.data_ptr(), n)

    def insert_ptr(self, src_ptr: int, dst_ptr: int, t_ptr: int, n: int) -> None:
        """insert() over device arrays given by address (int64 src / dst, float32 t): what the engine calls on rows of
        its event table.  The caller keeps the arrays alive and ordered on the current stream."""
        a = 0
        while a < n:
            m = min(max_chunk(self.capacity), n - a)
            self._make_room(m)
            _lib.call("tgnx_pairset_insert", _p(self.table), self.capacity, src_ptr + a * 8, dst_ptr + a * 8,
                      t_ptr + a * 4, m, self.num_nodes, _p(self.status), self._stream())
            a += m

    def erase_nodes(self, ids) -> int:
        """Erase every pair that names a node of `ids` as source or destination (a rehash with drop flags into a table
        of the same capacity; a uint8[num_nodes] flag array and the new table are allocated per call).  Returns the
        number of pairs erased.  Three host reads: the id validation, n_keys before and n_keys after."""
        ids = self._ids(ids)
        if ids.numel() == 0:
            return 0
        if bool(((ids < 0) | (ids >= self.num_nodes)).any()):
            raise ValueError(f"PairSet.erase_nodes: node ids must be in [0, {self.num_nodes})")
        drop = torch.zeros(self.num_nodes, dtype=torch.uint8, device=self.device)
        drop[ids] = 1
        before = self.n_keys
        self._rehash(self.capacity, drop)
        after = self.n_keys
        self._ub = after
        return before - after

    # ------------------------------------------------------------------ queries
    def _since(self, since, n: int, what: str):
        """(device float32[n] or None, the scalar cut) of a `since` argument."""
        if since is None:
            return None, float("-inf")
        if torch.is_tensor(since) or isinstance(since, np.ndarray):
            cut = torch.as_tensor(since).to(self.device, torch.float32).contiguous().view(-1)
            if int(cut.numel()) != n:
                raise ValueError(f"PairSet.{what}: one cut per query ({int(cut.numel())} for {n})")
            return cut, 0.0
        return None, float(np.float32(since))

    def lookup(self, src, dst, since=None):
        """(seen bool[n], count int64[n], t_first float32[n], t_last float32[n]) of the pairs (src[i], dst[i]).
        seen = present and t_last >= since (a float for every query, a tensor of n cuts, or None: present at all);
        the other three ignore the cut, and are 0 / +inf / -inf for an absent pair.  No host read."""
        src, dst = self._ids(src), self._ids(dst)
        n = int(src.numel())
        if int(dst.numel()) != n:
            raise ValueError("PairSet.lookup: src and dst differ in length")
        cut, cut_all = self._since(since, n, "lookup")
        seen = torch.empty(n, dtype=torch.bool, device=self.device)
        count = torch.empty(n, dtype=torch.int64, device=self.device)
        tf = torch.empty(n, dtype=torch.float32, device=self.device)
        tl = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.call("tgnx_pairset_lookup", _p(self.table), self.capacity, self.num_nodes, _p(src), _p(dst), n, _p(cut),
                  cut_all, _p(seen), _p(count), _p(tf), _p(tl), self._stream())
        return seen, count, tf, tl

    def contains(self, src, dst, since=None) -> torch.Tensor:
        """bool[n]: lookup()'s `seen` alone."""
        src, dst = self._ids(src), self._ids(dst)
        n = int(src.numel())
        if int(dst.numel()) != n:
            raise ValueError("PairSet.contains: src and dst differ in length")
        cut, cut_all = self._since(since, n, "contains")
        seen = torch.empty(n, dtype=torch.bool, device=self.device)
        _lib.call("tgnx_pairset_lookup", _p(self.table), self.capacity, self.num_nodes, _p(src), _p(dst), n, _p(cut),
                  cut_all, _p(seen), 0, 0, 0, self._stream())
        return seen

    def select(self, src, candidates, since=None):
        """For every source the candidates it has met (t_last >= since: a float, a tensor of one cut per source, or
        None), as a ragged (ptr int64[Q + 1], node ids): candidate order, duplicated candidates kept — what
        ops.link_topk / link_rank / embed_knn take as `exclude` once each segment is sorted.  Count pass, scan, fill
        pass; no [Q, C] intermediate; bit-identical between runs.  One host read (ptr[Q] sizes the ids)."""
        src, cand = self._ids(src), self._ids(candidates)
        Q, C = int(src.numel()), int(cand.numel())
        cut, cut_all = self._since(since, Q, "select")
        nb = int(_lib.lib().tgnx_pairset_select_ws_bytes(Q, C))
        if nb == 0:
            raise ValueError(f"PairSet.select: {Q} sources x {C} candidates are beyond one call")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        ptr = torch.empty(Q + 1, dtype=torch.int64, device=self.device)
        _lib.call("tgnx_pairset_select_count", _p(self.table), self.capacity, self.num_nodes, _p(src), Q, _p(cand), C,
                  _p(cut), cut_all, _p(ptr), _p(ws), ctypes.c_size_t(nb), self._stream())
        total = int(ptr[Q])
        ids = torch.empty(total, dtype=torch.int64, device=self.device)
        _lib.call("tgnx_pairset_select_fill", _p(self.table), self.capacity, self.num_nodes, _p(src), Q, _p(cand), C,
                  _p(cut), cut_all, _p(ids), total, _p(ws), ctypes.c_size_t(nb), self._stream())
        return ptr, ids

    # ------------------------------------------------------------------ checkpoints
    def state(self) -> dict:
        """The contents sorted by key: {"format", "num_nodes", "keys" int64[n] = src << 32 | dst ascending, "count"
        int64[n], "t_first" / "t_last" float32[n]} on the device.  The sorted form is the checkpoint and the only
        form two sets should be compared in.  One host read."""
        nk = self.n_keys
        keys = torch.empty(nk, dtype=torch.int64, device=self.device)
        count = torch.empty(nk, dtype=torch.int64, device=self.device)
        tf = torch.empty(nk, dtype=torch.float32, device=self.device)
        tl = torch.empty(nk, dtype=torch.float32, device=self.device)
        out_n = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.call("tgnx_pairset_export", _p(self.table), self.capacity, _p(keys), _p(count), _p(tf), _p(tl), nk,
                  _p(out_n), self._stream())
        keys, order = torch.sort(keys)
        return dict(format=STATE_FORMAT, num_nodes=self.num_nodes, keys=keys, count=count[order], t_first=tf[order],
                    t_last=tl[order])

    def load_state(self, state: dict) -> None:
        """Replace the contents by a state() dict's (its num_nodes may be smaller than this set's).  The capacity
        becomes the smallest that holds the rows at load <= 1/4, and never shrinks.  The rows are imported into a
        fresh table that replaces the set's only when every row was taken: RuntimeError, with the set unchanged, when
        one is refused (an id out of range, a count outside [1, 2^32), a NaN stamp, a duplicate key).  One host read."""
        n = check_state(state)
        if int(state["num_nodes"]) > self.num_nodes:
            raise ValueError(f"PairSet.load_state: the state has {int(state['num_nodes'])} nodes, this set {self.num_nodes}")
        cap = max(self.capacity, grown_capacity(n, MIN_CAPACITY))
        keys = state["keys"].to(self.device, torch.int64).contiguous()
        count = state["count"].to(self.device, torch.int64).contiguous()
        tf = state["t_first"].to(self.device, torch.float32).contiguous()
        tl = state["t_last"].to(self.device, torch.float32).contiguous()
        table = self._new_table(cap)
        status = torch.zeros(3, dtype=torch.int64, device=self.device)
        _lib.call("tgnx_pairset_import", _p(table), cap, _p(keys), _p(count), _p(tf), _p(tl), n, self.num_nodes,
                  _p(status), self._stream())
        c = dict(zip(("n_keys", "n_invalid", "n_overflow"), status.tolist()))
        if c["n_invalid"] or c["n_overflow"] or c["n_keys"] != n:
            raise RuntimeError(f"PairSet.load_state: {n} rows gave {c} (ids out of range, bad counts / stamps or "
                               "duplicate keys); the set is unchanged")
        self.table, self.capacity, self.status, self._ub = table, int(cap), status, n

    def to_pair_history(self):
        """A tgnx.tgb_negs.PairHistory-shaped CSR of the held pairs (indptr, each source's destinations ascending)
        from the sorted keys.  `first` is None: the set stores no rows, so contains(before=row) is not available;
        the CSR serves consumers that read indptr / indices."""
        from .tgb_negs import PairHistory
        keys = self.state()["keys"]
        s = keys >> 32
        indptr = torch.searchsorted(s, torch.arange(self.num_nodes + 1, device=self.device))
        return PairHistory(indptr, keys & 0xFFFFFFFF, None, 0)
