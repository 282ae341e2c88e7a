"""A numpy restatement of the embedding table's dependency rule (include/tgnx.h), and the oracle's
score-free state update, for tests/test_embtab_cpu.py and tests/test_gpu_embtab.py.

With T the nodes whose memory, last_update or ring row was written since the table was current, and ring(v) the
entries of v's ring row whose e_id is >= 0 (reset_state leaves stale ids in `neighbors`):
  D1 = { v : ring(v) meets T },  D2 = { v : ring(v) meets T | D1 },
  stale = T | D1 at layers = 1,  T | D1 | D2 at layers = 2,
on the ring as it stands when the list is made."""
import numpy as np
import torch


def _hop(neighbors, e_id, marked):
    """Nodes with a valid ring slot naming a marked node."""
    N = neighbors.shape[0]
    ok = (e_id >= 0) & (neighbors >= 0) & (neighbors < N)
    hit = np.zeros(neighbors.shape, dtype=bool)
    hit[ok] = marked[neighbors[ok]]
    return hit.any(axis=1)


def stale_ids(neighbors, e_id, touched, layers):
    """Ascending int64 ids of the stale rows.  neighbors, e_id: [N, K] integer arrays; touched: ids (any shape,
    duplicates allowed; ids outside [0, N) are ignored, as the touch kernel skips them)."""
    neighbors, e_id = np.asarray(neighbors), np.asarray(e_id)
    N = neighbors.shape[0]
    touched = np.asarray(touched, dtype=np.int64).reshape(-1)
    t = np.zeros(N, dtype=bool)
    t[touched[(touched >= 0) & (touched < N)]] = True
    d1 = _hop(neighbors, e_id, t)
    stale = t | d1
    if layers == 2:
        stale = stale | _hop(neighbors, e_id, t | d1)
    return np.flatnonzero(stale).astype(np.int64)


@torch.no_grad()
def oracle_observe(ref, lref, s, ev_t, ev_msg, lo, hi):
    """The oracle's update_state + ring insert of event rows [lo, hi) in eval mode (what eval_step leaves for any
    negatives; TgnEngine.observe's counterpart)."""
    ref.eval()
    src, dst = torch.from_numpy(s.src[lo:hi]), torch.from_numpy(s.dst[lo:hi])
    ref.memory.update_state(src, dst, ev_t[lo:hi], ev_msg[lo:hi])
    lref.insert(src.numpy(), dst.numpy(), ev_t[lo:hi].numpy())
