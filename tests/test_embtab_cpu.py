"""CPU checks of the embedding table's dependency rule (tests/embtab_ref.py; include/tgnx.h).

  hand cases   the numpy restatement on rings written by hand: an empty ring, a stale id under e_id = -1 that must not
               count, a 2-hop chain w -> u -> v, a touched node whose ring no longer holds its old neighbour;
  the rule     on the oracle (the setup of tests/test_gpu_tgn_query.py: 300 nodes, 600 events, d = 16, D = 32, ring 10;
               layers 1 and 2): after six eval batches one more batch is taken into the oracle's state.  Every node
               outside the reference's stale set keeps its oracle_embed row within 1e-6 in the `_close` metric (exact
               equality is expected: the margin covers CPU GEMM row placement only), and at least half of the touched
               nodes move by more than 100 x 2e-5 in that metric — which is what lets the GPU comparison at 2e-5
               (tests/test_gpu_embtab.py) see a row that was left stale.  The stream / parameter seeds are those of
               test_gpu_tgn_query.py (5 / 0): the precondition holds for them, so the GPU tests use the same;
  surface      the C entry points are declared and bound; the Python surface exists with the table off by default."""
import inspect

import numpy as np
import pytest
import torch

from embtab_ref import oracle_observe, stale_ids
from tgn_oracle_steps import oracle_embed

N, B, KN = 300, 50, 5
MOVE = 100 * 2e-5


def test_reference_on_an_empty_ring():
    nbr = np.full((6, 3), -1, dtype=np.int64)
    eid = np.full((6, 3), -1, dtype=np.int64)
    for layers in (1, 2):
        assert stale_ids(nbr, eid, [4, 1, 4], layers).tolist() == [1, 4]
        assert stale_ids(nbr, eid, [], layers).tolist() == []
        assert stale_ids(nbr, eid, [-1, 6, 2], layers).tolist() == [2]          # ids out of range are skipped


def test_reference_ignores_a_stale_id_under_a_reset_slot():
    nbr = np.full((5, 2), -1, dtype=np.int64)
    eid = np.full((5, 2), -1, dtype=np.int64)
    nbr[0] = [3, 3]          # reset_state left the ids: the slots are invalid
    nbr[1], eid[1] = [3, -1], [7, -1]
    for layers in (1, 2):
        assert stale_ids(nbr, eid, [3], layers).tolist() == [1, 3]


def test_reference_two_hop_chain():
    # ring(u) holds w, ring(v) holds u: touching w stales u at one hop, v only at two
    w, u, v = 0, 1, 2
    nbr = np.full((4, 2), -1, dtype=np.int64)
    eid = np.full((4, 2), -1, dtype=np.int64)
    nbr[u, 0], eid[u, 0] = w, 10
    nbr[v, 1], eid[v, 1] = u, 11
    assert stale_ids(nbr, eid, [w], 1).tolist() == [w, u]
    assert stale_ids(nbr, eid, [w], 2).tolist() == [w, u, v]
    assert stale_ids(nbr, eid, [v], 2).tolist() == [v]


def test_reference_a_touched_node_that_lost_its_old_neighbour():
    # a's ring used to hold b; the batch that touched a overwrote the slot with c.  b's row never named a, so b is
    # clean; a is stale as a touched node, c as the other endpoint
    a, b, c = 0, 1, 2
    nbr = np.full((3, 1), -1, dtype=np.int64)
    eid = np.full((3, 1), -1, dtype=np.int64)
    nbr[a, 0], eid[a, 0] = c, 21
    nbr[c, 0], eid[c, 0] = a, 21
    for layers in (1, 2):
        assert stale_ids(nbr, eid, [a, c], layers).tolist() == [a, c]
    nbr[b, 0], eid[b, 0] = a, 5                                                  # ... but a node that names a is not
    assert stale_ids(nbr, eid, [a, c], 1).tolist() == [a, b, c]


def _node_err(a, b):
    """The `_close` metric per row: max |a - b| over max(|b|.max(), 1)."""
    scale = max(float(b.abs().max()), 1.0)
    return ((a.double() - b.double()).abs().max(dim=1).values / scale).numpy()


@pytest.mark.parametrize("layers", [1, 2])
def test_the_rule_on_the_oracle(layers):
    from test_gpu_tgn_query import _negs, _oracle_state, _ref, _stream
    s = _stream()
    ref = _ref(layers, "last")
    lref, ev_t, ev_msg = _oracle_state(ref, s, _negs(s, B, KN), B, 6)
    allv = np.arange(N)
    before = oracle_embed(ref, lref, ev_t, ev_msg, allv).clone()
    oracle_observe(ref, lref, s, ev_t, ev_msg, 6 * B, 7 * B)
    after = oracle_embed(ref, lref, ev_t, ev_msg, allv)
    touched = np.unique(np.concatenate([s.src[6 * B:7 * B], s.dst[6 * B:7 * B]]))
    stale = stale_ids(lref.neighbors, lref.e_id, touched, layers)
    assert 0 < touched.size <= stale.size < N
    err = _node_err(after, before)
    clean = np.setdiff1d(allv, stale)
    moved = int((err[touched] > MOVE).sum())
    print(f"layers {layers}: touched {touched.size} stale {stale.size} clean max err {err[clean].max():.3e} "
          f"touched moved {moved} (min {err[touched].min():.3e}, median {np.median(err[touched]):.3e})")
    assert err[clean].max() <= 1e-6
    assert 2 * moved >= touched.size
    if layers == 2:                     # the second hop is not vacuous on this fixture
        assert stale.size > stale_ids(lref.neighbors, lref.e_id, touched, 1).size


def test_c_abi_and_python_surface():
    import pyg_epoch_utils
    from tgnx import _lib, tgn_epoch
    from tgnx.tgn import TgnEngine
    L = _lib.lib()
    for name in ("tgnx_embtab_touch", "tgnx_embtab_expand", "tgnx_embtab_list", "tgnx_embtab_list_ws_bytes",
                 "tgnx_tgn_embed_into"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.tgnx_embtab_list_ws_bytes(300) >= 2 * 4 and L.tgnx_embtab_list_ws_bytes(0) == 0
    assert L.tgnx_embtab_list_ws_bytes(1 << 31) == 0
    # refused before any device work: a bad node count, a null config
    assert L.tgnx_embtab_touch(None, None, 4, 0, None, None) == -1              # TGNX_EINVAL
    assert L.tgnx_embtab_expand(None, None, None, None) == -1
    assert L.tgnx_tgn_embed_into(None, None, None, 0, None, None) == -1
    for fn in ("enable_embedding_table", "disable_embedding_table", "refresh_embeddings", "embedding_table",
               "invalidate_embeddings", "embed_cached", "recommend_cached", "score_cached"):
        assert callable(getattr(TgnEngine, fn)), fn
    for fn in (TgnEngine.recommend_filtered, TgnEngine.rank, TgnEngine.rank_events, tgn_epoch.recommend_filtered,
               tgn_epoch.rank_stream):
        assert inspect.signature(fn).parameters["cached"].default is False, fn
    assert pyg_epoch_utils.embedding_table is tgn_epoch.embedding_table
