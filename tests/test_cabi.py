"""CPU checks of the C-ABI library: it loads, exports every declared symbol, and its host-side
entry points (no GPU needed) match the oracle / goldens."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def _declared():
    hdr = open(os.path.join(ROOT, "include", "tgnx.h")).read()
    return sorted(set(re.findall(r"\b(tgnx_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from tgnx import _lib
    L = _lib.lib()
    names = _declared()
    assert len(names) >= 8
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, f"{n} declared in include/tgnx.h but not bound in tgnx/_lib.py"
    assert L.tgnx_version() >= 1


def test_block_ids_host_matches_golden(golden):
    from tgnx import _lib
    z = golden("blocks.npz")
    src = np.ascontiguousarray(z["src"])
    dst = np.ascontiguousarray(z["dst"])
    out = np.empty_like(src)
    rc = _lib.lib().tgnx_block_ids_host(src.ctypes.data, dst.ctypes.data, src.shape[0], int(z["batch"][0]),
                                        out.ctypes.data)
    assert rc == 0
    np.testing.assert_array_equal(out, z["blocks"])


def test_block_ids_host_rejects_bad_input():
    from tgnx import _lib
    src = np.array([1, -2], dtype=np.int64)
    out = np.empty_like(src)
    rc = _lib.lib().tgnx_block_ids_host(src.ctypes.data, src.ctypes.data, 2, 2, out.ctypes.data)
    assert rc != 0
    assert b"negative" in _lib.lib().tgnx_last_error()


def test_torch_ops_library_registers_every_op():
    """torch.ops.tgnx (csrc/tgnx_torch.cpp, TORCH_LIBRARY over the C ABI) loads without a GPU and
    registers its schemas; the host op (block_ids) runs and matches the oracle (dependencyGraph.py:8-49)."""
    import numpy as np
    import torch

    from oracle import blocks_ref
    from tgnx import ops
    ns = ops.load()
    for name in ops.OPS:
        assert hasattr(ns, name), name
    assert "Tensor(a!) assoc" in str(ns.ring_sample.default._schema)
    rng = np.random.default_rng(0)
    src, dst = rng.integers(0, 50, 600), rng.integers(0, 50, 600)
    got = ns.block_ids(torch.from_numpy(src), torch.from_numpy(dst), 200).numpy()
    assert np.array_equal(got, blocks_ref.block_ids(src, dst, 200))


def test_tgn_param_layout_refuses_widths_outside_the_domain():
    """check_cfg accepts every even mem_dim in [2, 128]; 0, an odd width, 130 and a negative one are refused with its
    message (tgnx_tgn_param_layout only computes offsets: no device), and a valid width afterwards is laid out as
    tgnx.tgn.param_shapes says.  tests/test_gpu_tgn_mem_dims.py compares the accepted range with the oracle."""
    from tgnx import _lib
    from tgnx.tgn import PARAM_ORDER, TgnConfig, param_shapes
    L = _lib.lib()

    def layout(D):
        cfg = TgnConfig(num_nodes=300, num_events=100, ring=10, mem_dim=D, msg_dim=16, heads=2, max_batch=50, max_neg=1,
                        aggr=0, dropout=0.0, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, layers=1, updater=0, emb_in_msg=0)
        off = (ctypes.c_int64 * (len(PARAM_ORDER) + 1))()
        return L.tgnx_tgn_param_layout(ctypes.byref(cfg), off), list(off)

    for D in (0, 7, 130, -2):
        rc, _ = layout(D)
        assert rc == -1, D                                                 # TGNX_EINVAL
        assert b"tgn: mem_dim must be even and <= 128" in L.tgnx_last_error(), D
    for D in (2, 6, 128):                                                  # the domain's ends, after the refusals
        rc, off = layout(D)
        assert rc == 0, D
        shapes = param_shapes(D, 16)
        blocks = sorted((o, o + int(np.prod(shapes[name])), name) for name, o in zip(PARAM_ORDER, off))
        assert blocks[0][0] == 0 and blocks[-1][1] <= off[-1], (D, blocks, off[-1])
        for (a0, a1, name), (b0, _, _) in zip(blocks, blocks[1:]):
            assert a1 <= b0, (D, name)                                     # no two tensors overlap
        assert all(a % 4 == 0 for a, _, _ in blocks), (D, blocks)          # every block starts 16-byte aligned


def test_tgnn_param_layout_refuses_widths_outside_the_domain():
    """The TGNN step's check_cfg accepts mem_dim in [1, 128], msg_dim >= 0 with msg_dim + mem_dim <= 320 and 8 heads;
    tgnx_tgnn_param_layout (offsets only: no device) refuses the rest with its message and afterwards lays the
    domain's corners out as tgnx.model.param_shapes says.  tests/test_gpu_tgnn_widths.py compares the accepted
    widths with the oracle."""
    from tgnx import _lib
    from tgnx.model import PARAM_ORDER, TgnnConfig, param_shapes
    L = _lib.lib()

    def layout(D, d, heads=8):
        cfg = TgnnConfig(num_nodes=300, ring=10, mem_dim=D, msg_dim=d, heads=heads, max_batch=150, max_neg=8,
                         feat_drop=0.0, attn_drop=0.0, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
        off = (ctypes.c_int64 * (len(PARAM_ORDER) + 1))()
        return L.tgnx_tgnn_param_layout(ctypes.byref(cfg), off), list(off)

    for D, d, heads, msg in ((0, 16, 8, b"tgnn: mem_dim must be in [1, 128]"),
                             (129, 16, 8, b"tgnn: mem_dim must be in [1, 128]"),
                             (100, -1, 8, b"tgnn: msg_dim + mem_dim must be <= 320"),
                             (128, 193, 8, b"tgnn: msg_dim + mem_dim must be <= 320"),
                             (100, 16, 4, b"tgnn: heads must be 8")):
        rc, _ = layout(D, d, heads)
        assert rc == -1, (D, d, heads)                                     # TGNX_EINVAL
        assert msg in L.tgnx_last_error(), (D, d, heads, L.tgnx_last_error())
    for D, d in ((1, 0), (1, 319), (3, 0), (128, 0), (128, 192)):          # the domain's corners, after the refusals
        rc, off = layout(D, d)
        assert rc == 0, (D, d)
        shapes = param_shapes(D, d, 8)
        blocks = sorted((o, o + int(np.prod(shapes[name])), name) for name, o in zip(PARAM_ORDER, off))
        assert blocks[0][0] == 0 and blocks[-1][1] <= off[-1], (D, d, blocks, off[-1])
        for (a0, a1, name), (b0, _, _) in zip(blocks, blocks[1:]):
            assert a1 <= b0, (D, d, name)                                  # no two tensors overlap
        assert all(a % 4 == 0 for a, _, _ in blocks), (D, d, blocks)       # every block starts 16-byte aligned
