"""A numpy restatement of forgetting nodes (include/tgnx.h), for tests/test_forget_cpu.py and
tests/test_gpu_tgn_forget.py.  No device, no library.

A host snapshot h is a dict of arrays: the ring nbr / eid [N, K] int64 and rt [N, K] float32, the message stores
nodes [N, 4] = {s_off, s_cnt, d_off, d_cnt} and arena (tests/compact_ref.py), the event table src / dst / t, and
memory [N, D], last_update [N], node_gen [N].  With F the set of ids:

  own rows, v in F       memory 0, last_update 0, node_gen 0, node words {0, 0, 0, 0}, ring row -1 / -1 / -1.0;
  ring rows, u not in F  a slot is valid when eid >= 0 and nbr != -1.  Valid slots naming F are removed, the surviving
                         (eid, nbr) pairs keep their order at the front, every other slot is (-1, -1); rt becomes
                         t[eid] of the survivors sorted descending (stable: ties by slot), -1.0 behind.  A row that
                         loses nothing is unchanged (stale values under eid = -1 included);
  store runs, u not in F an entry e of the s run goes when dst[e] is in F, of the d run when src[e] is; survivors are
                         packed at the front of the same run in order, cnt reduced, off kept ({0, 0} when emptied);
                         arena words behind a shortened run keep their values;
  nothing else changes."""
import numpy as np
import torch


def _ids(ids, N):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= N):
        raise ValueError(f"node ids must be in [0, {N})")
    inF = np.zeros(N, dtype=bool)
    inF[ids] = True
    return inF


def ring_forget(nbr, eid, rt, ids, ev_t=None):
    """The ring part: returns (nbr, eid, rt, counts) as new arrays.  ev_t None (a loader without an event table): rt
    drops the slots eid drops."""
    nbr, eid, rt = np.array(nbr, dtype=np.int64), np.array(eid, dtype=np.int64), np.array(rt, dtype=np.float32)
    N, K = nbr.shape
    inF = _ids(ids, N)
    slots = rows = 0
    for u in range(N):
        if inF[u]:
            nbr[u], eid[u], rt[u] = -1, -1, np.float32(-1.0)
            continue
        valid = (eid[u] >= 0) & (nbr[u] != -1)
        gone = valid.copy()
        gone[valid] = inF[nbr[u][valid]]
        if not gone.any():
            continue
        slots += int(gone.sum())
        rows += 1
        keep = np.flatnonzero(valid & ~gone)
        s = keep.size
        e_new, n_new = np.full(K, -1, np.int64), np.full(K, -1, np.int64)
        t_new = np.full(K, -1.0, np.float32)
        e_new[:s], n_new[:s] = eid[u][keep], nbr[u][keep]
        if ev_t is None:
            t_new[:s] = rt[u][keep]
        else:
            tt = np.asarray(ev_t, dtype=np.float32)[eid[u][keep]]
            t_new[:s] = tt[np.argsort(-tt, kind="stable")]
        nbr[u], eid[u], rt[u] = n_new, e_new, t_new
    return nbr, eid, rt, dict(nodes=int(inF.sum()), ring_slots=slots, ring_rows=rows)


def forget_ref(h, ids):
    """(h2, counts): the snapshot after forget_nodes(ids) — a new dict whose changed arrays are copies — and the counts
    TgnEngine.forget_nodes returns."""
    N = h["nbr"].shape[0]
    inF = _ids(ids, N)
    out = dict(h)
    out["nbr"], out["eid"], out["rt"], counts = ring_forget(h["nbr"], h["eid"], h["rt"], ids, ev_t=h["t"])
    nodes, arena = np.array(h["nodes"], dtype=np.int64), np.array(h["arena"], dtype=np.int64)
    entries = 0
    for u in range(N):
        if inF[u]:
            nodes[u] = 0
            continue
        for c, partner in ((0, h["dst"]), (2, h["src"])):
            off, cnt = int(nodes[u, c]), int(nodes[u, c + 1])
            if cnt == 0:
                continue
            run = arena[off:off + cnt].copy()
            keep = ~inF[np.asarray(partner)[run]]
            k = int(keep.sum())
            if k == cnt:
                continue
            entries += cnt - k
            arena[off:off + k] = run[keep]
            nodes[u, c], nodes[u, c + 1] = (off if k else 0), k
    out["nodes"], out["arena"] = nodes, arena
    for key in ("memory", "last_update", "node_gen"):
        x = np.array(h[key])
        x[inF] = 0
        out[key] = x
    counts["store_entries"] = entries
    return out, counts


def names_forgotten(h, ids):
    """Whether any valid ring slot or store run of the snapshot still names an event with an endpoint in ids."""
    N = h["nbr"].shape[0]
    inF = _ids(ids, N)
    valid = (h["eid"] >= 0) & (h["nbr"] != -1)
    e = h["eid"][valid]
    if (inF[h["nbr"][valid]]).any() or (inF[h["src"][e]] | inF[h["dst"][e]]).any():
        return True
    for so, sc, do, dc in np.asarray(h["nodes"]).tolist():
        for off, cnt in ((so, sc), (do, dc)):
            run = h["arena"][off:off + cnt]
            if (inF[h["src"][run]] | inF[h["dst"][run]]).any():
                return True
    return False


@torch.no_grad()
def oracle_forget(ref, lref, ids, ev_t):
    """The rule applied to the oracle (oracle/tgn_ref.py RefTGN, oracle/sampler_ref.py RefLastNeighborLoader): memory
    and last_update rows, msg_s_store / msg_d_store (entry = (node, partner, t, raw): keyed by the node, dropped by
    the partner) and the loader's rows.  ev_t: the event table's t, a float32 array indexed by e_id."""
    mem = ref.memory
    N = mem.memory.shape[0]
    inF = _ids(ids, N)
    F = torch.from_numpy(np.flatnonzero(inF))
    mem.memory[F] = 0
    mem.last_update[F] = 0
    for store in (mem.msg_s_store, mem.msg_d_store):
        for u in list(store):
            if inF[u]:
                del store[u]
                continue
            keep = ~torch.isin(store[u][1], F)
            if bool(keep.all()):
                continue
            if bool(keep.any()):
                store[u] = tuple(x[keep] for x in store[u])
            else:
                del store[u]
    lref.neighbors, lref.e_id, lref.t, _ = ring_forget(lref.neighbors, lref.e_id, lref.t, ids, ev_t=np.asarray(ev_t))


# ---------------------------------------------------------------------------------------------- streams and a simulator
def make_events(seed, nev, N, d, lo=0):
    """A time-ordered random stream over nodes [lo, N): src, dst uniform (self loops occur), t ascending with ties,
    msg float32 [nev, d]."""
    g = np.random.default_rng(seed)
    return dict(src=g.integers(lo, N, nev).astype(np.int64), dst=g.integers(lo, N, nev).astype(np.int64),
                t=np.cumsum(g.integers(0, 3, nev)).astype(np.float32),
                msg=g.standard_normal((nev, d)).astype(np.float32))


def component_events(seed, nev, d, n_main=60, N=70, share=0.2):
    """make_events over [0, n_main) in which a random `share` of the rows is rewritten to run between nodes of
    [n_main, N) only: two components, interleaved in time.  Returns (events, mask of the component's rows)."""
    ev = make_events(seed, nev, n_main, d)
    g = np.random.default_rng(seed + 1)
    comp = g.random(nev) < share
    k = int(comp.sum())
    ev["src"][comp], ev["dst"][comp] = g.integers(n_main, N, k), g.integers(n_main, N, k)
    return ev, comp


def hub_events(seed, N, d, hub=7, B=200):
    """One batch of B = 200 events in which `hub` is the source of 150 events and the destination of 70 (20 of them
    self loops): its s run spans three 64-entry chunks, its d run two; preceded by one ordinary batch."""
    ev = make_events(seed, 2 * B, N, d)
    src, dst = ev["src"], ev["dst"]
    src[src == hub] = hub + 1                      # (the hub occurs in the second batch only)
    dst[dst == hub] = hub + 2
    src[B:B + 150] = hub
    dst[B + 130:B + 200] = hub
    return ev


def simulate(ev, B, N, K):
    """The host snapshot (keys of forget_ref, without memory / last_update / node_gen values: zeros) that observing
    the stream in batches of B leaves: the ring by the oracle's loader, the stores by their definition — the batch at
    row s owns arena words [2s, 2s + 2B), its rows sorted stably by src, then by dst; a node's run is its slice."""
    from oracle.sampler_ref import RefLastNeighborLoader
    src, dst, t = ev["src"], ev["dst"], ev["t"].astype(np.float32)
    nev = src.shape[0]
    ld = RefLastNeighborLoader(N, K)
    nodes, arena = np.zeros((N, 4), np.int64), np.zeros(2 * nev, np.int64)
    for s in range(0, nev, B):
        e = np.arange(s, min(s + B, nev))
        ld.insert(src[e], dst[e], t[e])
        for c, key, base in ((0, src, 2 * s), (2, dst, 2 * s + e.size)):
            order = e[np.argsort(key[e], kind="stable")]
            arena[base:base + e.size] = order
            u, first, cnt = np.unique(key[order], return_index=True, return_counts=True)
            nodes[u, c], nodes[u, c + 1] = base + first, cnt
    return dict(nbr=ld.neighbors.copy(), eid=ld.e_id.copy(), rt=ld.t.copy(), nodes=nodes, arena=arena, src=src, dst=dst,
                t=t, msg=ev["msg"], memory=np.zeros((N, 4), np.float32), last_update=np.zeros(N, np.int64),
                node_gen=np.zeros(N, np.int32))
