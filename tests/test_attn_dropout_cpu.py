"""Attention dropout of the per-operator layer, the parts that need no GPU: the torch ops' registration, the C entry
points' argument check (before any device call), the Python-side seed rules, and that the cases of
test_gpu_attn_dropout.py cannot pass vacuously (from tests/dropout_ref.py and the oracle alone).

Measured over the 16 (shape, key mode, p) cases: dropped shares 0.095 .. 0.106 at p = 0.1 and 0.490 .. 0.516 at
p = 0.5; the mask moves the oracle's output by 0.72 .. 1.0 in close()'s measure (bound: > 2e-3)."""
import ctypes

import numpy as np
import pytest
import torch

import attn_dropout_cases as A
import dropout_ref as dr


def test_torch_ops_are_listed_and_registered():
    from tgnx import ops
    ns = ops.load()
    for name in ("edge_attn_drop_fwd", "edge_attn_drop_bwd"):
        assert name in ops.OPS, name
        assert hasattr(ns, name), name
        schema = str(getattr(ns, name).default._schema)
        assert "Tensor? dst_key" in schema and "Tensor? edge_key" in schema, schema
        assert "float p, int seed, int stream" in schema, schema
    assert ops.ATTN_DROPOUT_STREAM == 7


@pytest.mark.parametrize("p", [-0.1, 1.0, float("nan"), float("inf")])
def test_entry_points_refuse_bad_p_before_any_device_call(p):
    """Host pointers that are never touched; the call fails in its argument check (no HIP call is made)."""
    from tgnx import _lib
    L = _lib.lib()
    a = np.zeros(64, dtype=np.float32)
    ptr, null = ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(0)
    rc = L.tgnx_edge_attn_drop_fwd(2, 3, 2, 4, ptr, ptr, ptr, ptr, ptr, ptr, ptr, p, 1, 7, null, null, null)
    assert rc != 0 and b"tgnx_edge_attn_drop_fwd" in L.tgnx_last_error() and b"p must be" in L.tgnx_last_error()
    rc = L.tgnx_edge_attn_drop_bwd(2, 3, 2, 4, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, p, 1, 7, null,
                                   null, null)
    assert rc != 0 and b"tgnx_edge_attn_drop_bwd" in L.tgnx_last_error() and b"p must be" in L.tgnx_last_error()
    assert a.sum() == 0


def test_entry_points_check_sizes_as_the_plain_pair():
    from tgnx import _lib
    L = _lib.lib()
    a = np.zeros(64, dtype=np.float32)
    ptr, null = ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(0)
    rc = L.tgnx_edge_attn_drop_fwd(2, 3, 9, 4, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0.1, 1, 7, null, null, null)
    assert rc != 0 and b"tgnx_edge_attn_drop_fwd: bad sizes" in L.tgnx_last_error()
    rc = L.tgnx_edge_attn_fwd(2, 3, 9, 4, ptr, ptr, ptr, ptr, ptr, ptr, ptr, null)
    assert rc != 0 and b"tgnx_edge_attn_fwd: bad sizes" in L.tgnx_last_error()


def test_edge_attention_with_dropout_needs_a_seed():
    from tgnx.ops import edge_attention
    q, k = torch.zeros(2, 8), torch.zeros(3, 8)
    indptr = torch.tensor([0, 1, 3])
    with pytest.raises(ValueError, match="seed"):
        edge_attention(q, k, k, None, indptr, 2, dropout=0.1)
    with pytest.raises(ValueError, match="seed"):
        edge_attention(q, k, k, None, indptr, 2, dropout=0.1, seed=-1)
    with pytest.raises(ValueError, match="seed"):
        edge_attention(q, k, k, None, indptr, 2, dropout=0.1, seed=1 << 63)


def test_step_seed_is_the_engines():
    from tgnx.ops import step_seed
    for base, nb in [(0, 1), (11, 1), (11, 2), (20240607, 7), ((1 << 63) - 1, 123456789), (1 << 64, 3)]:
        assert step_seed(base, nb) == dr.step_seed(base & ((1 << 64) - 1), nb), (base, nb)
        assert 0 <= step_seed(base, nb) < (1 << 63)


def test_set_dropout_seed_counts_training_forwards():
    from tgnx.nn import GraphAttentionEmbedding, TimeEncoder, TransformerConv
    conv = TransformerConv(8, 4, heads=2, dropout=0.1, edge_dim=3).train()
    keys = list(conv.state_dict())
    assert conv.take_dropout_seed() is None
    conv.set_dropout_seed(11)
    assert list(conv.state_dict()) == keys                   # plain attributes, not buffers
    assert conv.take_dropout_seed() == dr.step_seed(11, 1)
    assert conv.take_dropout_seed() == dr.step_seed(11, 2)
    conv.set_dropout_seed(11)                                # again: the counter starts over
    assert conv.take_dropout_seed() == dr.step_seed(11, 1)
    conv.set_dropout_seed(None)                              # back to raising, before any device work
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.zeros(2, 8), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 3))
    gnn = GraphAttentionEmbedding(8, 8, 2, TimeEncoder(4))
    gnn.set_dropout_seed(5)
    assert gnn.conv.take_dropout_seed() == dr.step_seed(5, 1)


@pytest.mark.parametrize("H,C,with_e,mode,p", A.CASES)
def test_gpu_cases_are_not_vacuous(H, C, with_e, mode, p):
    s = A.assert_not_vacuous(A.case(H, C, with_e, mode, p), p)
    print(f"H {H} C {C} {mode} p {p}: {s}")
    lo, hi = (0.095, 0.106) if p == 0.1 else (0.490, 0.516)
    assert lo - 5e-4 <= s["dropped"] <= hi + 5e-4, s        # the shares the cases were chosen with
